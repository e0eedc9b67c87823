// bp_gemm_bf16 / bp_gemm_f16: D[M,N] = A[M,K] . W[N,K]^T (+ bias[N]) (-> tanh-GELU) by a PINNED hipBLASLt solution.
// Host C++ only, no kernel of this repository.  See include/bp_hip.h for the contract.
//
// Which algorithm runs is a function of the caller's table alone: a row names a solution index of one library version
// on one architecture; the index is turned into an algorithm (hipblaslt_ext::getAlgosFromIndex), checked against the
// actual problem (hipblaslt_ext::matmulIsAlgoSupported) and run.  Every other outcome is a BP_GEMM_* status (> 0) and
// nothing is launched; the caller then takes its ordinary GEMM.  The heuristic is never asked here.
//
// The library is the libhipblaslt the process has ALREADY loaded (PyTorch brings one): it is looked up with
// dlopen(RTLD_NOLOAD) and its entry points with dlsym, so this file adds no DT_NEEDED entry and can never bring a second
// copy into the process.  Without a loaded libhipblaslt every call answers BP_GEMM_NO_LIBRARY.
#include <dlfcn.h>
#include <hip/hip_runtime.h>
#include <hipblaslt/hipblaslt.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <map>
#include <mutex>
#include <vector>

#include "../../include/bp_hip.h"

namespace {

constexpr size_t kWorkspaceBytes = size_t(128) << 20;   // sized once per device: stream-K solutions need one
constexpr int kMaxDevices = 64;

// ---- the loaded library ------------------------------------------------------------------------------------------------
struct Lt {
    decltype(&hipblasLtCreate) create = nullptr;
    decltype(&hipblasLtDestroy) destroy = nullptr;
    decltype(&hipblasLtGetVersion) get_version = nullptr;
    decltype(&hipblasLtMatmulDescCreate) desc_create = nullptr;
    decltype(&hipblasLtMatmulDescDestroy) desc_destroy = nullptr;
    decltype(&hipblasLtMatmulDescSetAttribute) desc_set = nullptr;
    decltype(&hipblasLtMatrixLayoutCreate) layout_create = nullptr;
    decltype(&hipblasLtMatrixLayoutDestroy) layout_destroy = nullptr;
    decltype(&hipblasLtMatmulPreferenceCreate) pref_create = nullptr;
    decltype(&hipblasLtMatmulPreferenceDestroy) pref_destroy = nullptr;
    decltype(&hipblasLtMatmulPreferenceSetAttribute) pref_set = nullptr;
    decltype(&hipblasLtMatmulAlgoGetHeuristic) heuristic = nullptr;
    decltype(&hipblasLtMatmul) matmul = nullptr;
    // hipblaslt_ext:: (C++ linkage: looked up by their mangled names)
    int (*index_from_algo)(hipblasLtMatmulAlgo_t &) = nullptr;
    hipblasStatus_t (*algos_from_index)(hipblasLtHandle_t, std::vector<int> &,
                                        std::vector<hipblasLtMatmulHeuristicResult_t> &) = nullptr;
    hipblasStatus_t (*is_algo_supported)(hipblasLtHandle_t, hipblasLtMatmulDesc_t, const void *, hipblasLtMatrixLayout_t,
                                         hipblasLtMatrixLayout_t, const void *, hipblasLtMatrixLayout_t,
                                         hipblasLtMatrixLayout_t, hipblasLtMatmulAlgo_t &, size_t &) = nullptr;
    bool ok = false;
};

template <class F>
bool sym(void *h, const char *name, F &fn) {
    fn = reinterpret_cast<F>(dlsym(h, name));
    return fn != nullptr;
}

const Lt &lt() {
    static const Lt loaded = [] {
        Lt l;
        void *h = nullptr;
        for (const char *name : {"libhipblaslt.so.1", "libhipblaslt.so", "libhipblaslt.so.0"}) {
            h = dlopen(name, RTLD_NOLOAD | RTLD_LAZY | RTLD_LOCAL);   // NOLOAD: only a copy the process already has
            if (h != nullptr) break;
        }
        if (h == nullptr) return l;
        l.ok = sym(h, "hipblasLtCreate", l.create) && sym(h, "hipblasLtDestroy", l.destroy) && sym(h, "hipblasLtGetVersion", l.get_version)
            && sym(h, "hipblasLtMatmulDescCreate", l.desc_create) && sym(h, "hipblasLtMatmulDescDestroy", l.desc_destroy)
            && sym(h, "hipblasLtMatmulDescSetAttribute", l.desc_set)
            && sym(h, "hipblasLtMatrixLayoutCreate", l.layout_create) && sym(h, "hipblasLtMatrixLayoutDestroy", l.layout_destroy)
            && sym(h, "hipblasLtMatmulPreferenceCreate", l.pref_create)
            && sym(h, "hipblasLtMatmulPreferenceDestroy", l.pref_destroy)
            && sym(h, "hipblasLtMatmulPreferenceSetAttribute", l.pref_set)
            && sym(h, "hipblasLtMatmulAlgoGetHeuristic", l.heuristic) && sym(h, "hipblasLtMatmul", l.matmul)
            && sym(h, "_ZN13hipblaslt_ext16getIndexFromAlgoER22_hipblasLtMatmulAlgo_t", l.index_from_algo)
            && sym(h, "_ZN13hipblaslt_ext17getAlgosFromIndexEPvRSt6vectorIiSaIiEERS1_I33_hipblasLtMatmulHeuristicResult_tSaIS5_EE",
                   l.algos_from_index)
            && sym(h, "_ZN13hipblaslt_ext21matmulIsAlgoSupportedEPvP27hipblasLtMatmulDescOpaque_tPKvP29hipblasLtMatrixLayout"
                      "Opaque_tS6_S4_S6_S6_R22_hipblasLtMatmulAlgo_tRm", l.is_algo_supported);
        return l;
    }();
    return loaded;
}

// ---- per-device state: created on first use, kept for the life of the process ---------------------------------------------
struct Device {
    std::mutex mu;
    bool ready = false;
    hipblasLtHandle_t handle = nullptr;
    void *workspace = nullptr;
    int version = 0;
    char arch[32] = {0};
    // the one workspace is ordered across streams: a launch that needs it waits for the last one that used it
    hipEvent_t ws_event = nullptr;
    hipStream_t ws_stream = nullptr;
    bool ws_used = false;
    // what the library answers for a solution index (found, algorithm): one entry per index a table has named
    std::map<int, std::pair<bool, hipblasLtMatmulAlgo_t>> algos;
};

Device g_devices[kMaxDevices];

// BP_OK, or BP_ERR_GEMM with everything that was created released again (the next call tries afresh; the reason is
// written to stderr once per process); the caller holds dev.mu
int device_init(Device &dev, int id) {
    if (dev.ready) return BP_OK;
    const Lt &l = lt();
    const char *what = nullptr;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, id) != hipSuccess) what = "hipGetDeviceProperties";
    else if (l.create(&dev.handle) != HIPBLAS_STATUS_SUCCESS) { what = "hipblasLtCreate"; dev.handle = nullptr; }
    else if (l.get_version(dev.handle, &dev.version) != HIPBLAS_STATUS_SUCCESS) what = "hipblasLtGetVersion";
    else if (hipMalloc(&dev.workspace, kWorkspaceBytes) != hipSuccess) { what = "hipMalloc of the workspace"; dev.workspace = nullptr; }
    else if (hipEventCreateWithFlags(&dev.ws_event, hipEventDisableTiming) != hipSuccess) { what = "hipEventCreate"; dev.ws_event = nullptr; }
    if (what != nullptr) {
        if (dev.workspace) (void)hipFree(dev.workspace);
        if (dev.handle) l.destroy(dev.handle);
        dev.workspace = nullptr;
        dev.handle = nullptr;
        static bool said = false;
        if (!said) fprintf(stderr, "bp_gemm: %s failed on device %d: pinned GEMM rows are not used\n", what, id);
        said = true;
        return BP_ERR_GEMM;
    }
    const char *colon = strchr(prop.gcnArchName, ':');   // "gfx950:sramecc+:xnack-" -> "gfx950"
    size_t n = colon ? size_t(colon - prop.gcnArchName) : strlen(prop.gcnArchName);
    if (n >= sizeof(dev.arch)) n = sizeof(dev.arch) - 1;
    memcpy(dev.arch, prop.gcnArchName, n);
    dev.arch[n] = 0;
    dev.ready = true;
    return BP_OK;
}

// ---- one problem's descriptors (destroyed on scope exit) -----------------------------------------------------------------
struct Problem {
    const Lt &l;
    hipblasLtMatmulDesc_t desc = nullptr;
    hipblasLtMatrixLayout_t w = nullptr, a = nullptr, d = nullptr;
    explicit Problem(const Lt &lib) : l(lib) {}
    ~Problem() {
        if (d) l.layout_destroy(d);
        if (a) l.layout_destroy(a);
        if (w) l.layout_destroy(w);
        if (desc) l.desc_destroy(desc);
    }
    // Row-major D[M,N] = A[M,K] W[N,K]^T is, column-major, D^T[N,M] = op_T(W as K x N, ld ldw) . (A as K x M, ld lda):
    // the library's m is N, its n is M, and the bias runs along the rows of its D, i.e. over N.
    bool make(int dtype, int epilogue, int64_t M, int N, int K, int64_t lda, int64_t ldw, int64_t ldd, const void *bias) {
        const hipDataType t = dtype == BP_DTYPE_BF16 ? HIP_R_16BF : HIP_R_16F;
        const int32_t op_t = HIPBLAS_OP_T, op_n = HIPBLAS_OP_N;
        bool ok = l.desc_create(&desc, HIPBLAS_COMPUTE_32F, HIP_R_32F) == HIPBLAS_STATUS_SUCCESS
            && l.desc_set(desc, HIPBLASLT_MATMUL_DESC_TRANSA, &op_t, sizeof(op_t)) == HIPBLAS_STATUS_SUCCESS
            && l.desc_set(desc, HIPBLASLT_MATMUL_DESC_TRANSB, &op_n, sizeof(op_n)) == HIPBLAS_STATUS_SUCCESS;
        if (ok && epilogue != BP_GEMM_EPILOGUE_NONE) {
            const uint32_t ep = epilogue == BP_GEMM_EPILOGUE_BIAS_GELU ? HIPBLASLT_EPILOGUE_GELU_BIAS : HIPBLASLT_EPILOGUE_BIAS;
            const int32_t bias_type = t;
            ok = l.desc_set(desc, HIPBLASLT_MATMUL_DESC_EPILOGUE, &ep, sizeof(ep)) == HIPBLAS_STATUS_SUCCESS
                && l.desc_set(desc, HIPBLASLT_MATMUL_DESC_BIAS_DATA_TYPE, &bias_type, sizeof(bias_type)) == HIPBLAS_STATUS_SUCCESS
                && l.desc_set(desc, HIPBLASLT_MATMUL_DESC_BIAS_POINTER, &bias, sizeof(bias)) == HIPBLAS_STATUS_SUCCESS;
        }
        return ok && l.layout_create(&w, t, uint64_t(K), uint64_t(N), ldw) == HIPBLAS_STATUS_SUCCESS
            && l.layout_create(&a, t, uint64_t(K), uint64_t(M), lda) == HIPBLAS_STATUS_SUCCESS
            && l.layout_create(&d, t, uint64_t(N), uint64_t(M), ldd) == HIPBLAS_STATUS_SUCCESS;
    }
};

int check_problem(int dtype, int epilogue, const void *a, const void *w, const void *bias, const void *d,
                  int64_t M, int N, int K, int64_t lda, int64_t ldw, int64_t ldd) {
    if (dtype != BP_DTYPE_F16 && dtype != BP_DTYPE_BF16) return BP_ERR_DTYPE;
    if (epilogue < BP_GEMM_EPILOGUE_NONE || epilogue > BP_GEMM_EPILOGUE_BIAS_GELU) return BP_ERR_SHAPE;
    if (a == nullptr || w == nullptr || d == nullptr || (epilogue != BP_GEMM_EPILOGUE_NONE) != (bias != nullptr)) return BP_ERR_SHAPE;
    if (M < 1 || N < 1 || K < 1 || lda < K || ldw < K || ldd < N) return BP_ERR_SHAPE;
    return BP_OK;
}

bool capturing(hipStream_t st) {
    hipStreamCaptureStatus status = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &status) != hipSuccess) return true;
    return status != hipStreamCaptureStatusNone;
}

// The row of `table` for this problem on this device: same dtype / epilogue / N / K, the largest m_min <= M.  A row of
// another library version or architecture that would otherwise have been chosen makes the answer BP_GEMM_VERSION.
int lookup(const bp_gemm_row *table, int n_rows, int dtype, int epilogue, int64_t M, int N, int K, const Device &dev,
           int &solution) {
    const bp_gemm_row *best = nullptr;
    for (int i = 0; i < n_rows; ++i) {
        const bp_gemm_row &r = table[i];
        if (r.dtype != dtype || r.epilogue != epilogue || r.n != N || r.k != K || r.m_min > M || r.m_min < 1) continue;
        if (best == nullptr || r.m_min > best->m_min) best = &r;
    }
    if (best == nullptr) return BP_GEMM_MISS;
    if (best->version != dev.version || strncmp(best->arch, dev.arch, sizeof(best->arch)) != 0) return BP_GEMM_VERSION;
    if (best->solution < 0) return BP_GEMM_MISS;    // a row that says "keep the heuristic"
    solution = best->solution;
    return BP_OK;
}

int gemm(int dtype, const void *a, const void *w, const void *bias, void *d, int64_t M, int N, int K,
         int64_t lda, int64_t ldw, int64_t ldd, int epilogue, const bp_gemm_row *table, int n_rows, int *solution_out,
         bp_stream_t stream) {
    if (solution_out) *solution_out = -1;
    int st = check_problem(dtype, epilogue, a, w, bias, d, M, N, K, lda, ldw, ldd);
    if (st != BP_OK) return st;
    if (n_rows < 0 || (n_rows > 0 && table == nullptr)) return BP_ERR_SHAPE;
    if (n_rows == 0) return BP_GEMM_MISS;
    hipStream_t hs = static_cast<hipStream_t>(stream);
    if (capturing(hs)) return BP_GEMM_CAPTURING;   // a first use allocates; a graph keeps its GEMMs on the ordinary path
    const Lt &l = lt();
    if (!l.ok) return BP_GEMM_NO_LIBRARY;
    int id = 0;
    if (hipGetDevice(&id) != hipSuccess || id < 0 || id >= kMaxDevices) return BP_ERR_GEMM;
    Device &dev = g_devices[id];
    std::lock_guard<std::mutex> lock(dev.mu);
    if ((st = device_init(dev, id)) != BP_OK) return st;
    int solution = -1;
    if ((st = lookup(table, n_rows, dtype, epilogue, M, N, K, dev, solution)) != BP_OK) return st;

    Problem p(l);
    if (!p.make(dtype, epilogue, M, N, K, lda, ldw, ldd, bias)) return BP_ERR_GEMM;
    const float alpha = 1.f, beta = 0.f;
    auto it = dev.algos.find(solution);
    if (it == dev.algos.end()) {
        std::pair<bool, hipblasLtMatmulAlgo_t> entry(false, hipblasLtMatmulAlgo_t{});
        std::vector<int> index(1, solution);
        std::vector<hipblasLtMatmulHeuristicResult_t> found;
        if (l.algos_from_index(dev.handle, index, found) == HIPBLAS_STATUS_SUCCESS && !found.empty()
            && found[0].state == HIPBLAS_STATUS_SUCCESS && l.index_from_algo(found[0].algo) == solution) {
            entry.first = true;
            entry.second = found[0].algo;
        }
        it = dev.algos.emplace(solution, entry).first;
    }
    if (!it->second.first) return BP_GEMM_UNSUPPORTED;
    hipblasLtMatmulAlgo_t algo = it->second.second;
    size_t need = 0;
    // every call: the check binds the algorithm to THIS problem's descriptors and says what workspace it needs
    if (l.is_algo_supported(dev.handle, p.desc, &alpha, p.w, p.a, &beta, p.d, p.d, algo, need) != HIPBLAS_STATUS_SUCCESS
        || need > kWorkspaceBytes)
        return BP_GEMM_UNSUPPORTED;
    if (need > 0 && dev.ws_used && dev.ws_stream != hs && hipStreamWaitEvent(hs, dev.ws_event, 0) != hipSuccess)
        return BP_ERR_GEMM;
    if (l.matmul(dev.handle, p.desc, &alpha, w, p.w, a, p.a, &beta, d, p.d, d, p.d, &algo, dev.workspace, kWorkspaceBytes, hs)
        != HIPBLAS_STATUS_SUCCESS)
        return BP_ERR_GEMM;
    if (need > 0) {
        if (hipEventRecord(dev.ws_event, hs) != hipSuccess) return BP_ERR_GEMM;
        dev.ws_stream = hs;
        dev.ws_used = true;
    }
    if (solution_out) *solution_out = solution;
    return BP_OK;
}

}  // namespace

extern "C" {

int bp_gemm_bf16(const void *a, const void *w, const void *bias, void *d, int64_t M, int N, int K,
                 int64_t lda, int64_t ldw, int64_t ldd, int epilogue, const bp_gemm_row *table, int n_rows,
                 int *solution_out, bp_stream_t stream) {
    return gemm(BP_DTYPE_BF16, a, w, bias, d, M, N, K, lda, ldw, ldd, epilogue, table, n_rows, solution_out, stream);
}

int bp_gemm_f16(const void *a, const void *w, const void *bias, void *d, int64_t M, int N, int K,
                int64_t lda, int64_t ldw, int64_t ldd, int epilogue, const bp_gemm_row *table, int n_rows,
                int *solution_out, bp_stream_t stream) {
    return gemm(BP_DTYPE_F16, a, w, bias, d, M, N, K, lda, ldw, ldd, epilogue, table, n_rows, solution_out, stream);
}

int bp_gemm_library(int *version, char *arch, int arch_len) {
    const Lt &l = lt();
    if (!l.ok) return BP_GEMM_NO_LIBRARY;
    int id = 0;
    if (hipGetDevice(&id) != hipSuccess || id < 0 || id >= kMaxDevices) return BP_ERR_GEMM;
    Device &dev = g_devices[id];
    std::lock_guard<std::mutex> lock(dev.mu);
    int st = device_init(dev, id);
    if (st != BP_OK) return st;
    if (version) *version = dev.version;
    if (arch && arch_len > 0) {
        strncpy(arch, dev.arch, size_t(arch_len) - 1);
        arch[arch_len - 1] = 0;
    }
    return BP_OK;
}

int bp_gemm_heuristic(int dtype, int epilogue, int64_t M, int N, int K, int64_t lda, int64_t ldw, int64_t ldd,
                      int *solutions, int max_solutions, int *count) {
    if (count) *count = 0;
    if (solutions == nullptr || count == nullptr || max_solutions < 1 || max_solutions > 1024) return BP_ERR_SHAPE;
    static const char dummy = 0;   // pointers are not read by the query; the bias only has to be there
    int st = check_problem(dtype, epilogue, &dummy, &dummy, epilogue != BP_GEMM_EPILOGUE_NONE ? &dummy : nullptr, &dummy,
                           M, N, K, lda, ldw, ldd);
    if (st != BP_OK) return st;
    const Lt &l = lt();
    if (!l.ok) return BP_GEMM_NO_LIBRARY;
    int id = 0;
    if (hipGetDevice(&id) != hipSuccess || id < 0 || id >= kMaxDevices) return BP_ERR_GEMM;
    Device &dev = g_devices[id];
    std::lock_guard<std::mutex> lock(dev.mu);
    if ((st = device_init(dev, id)) != BP_OK) return st;
    Problem p(l);
    if (!p.make(dtype, epilogue, M, N, K, lda, ldw, ldd, epilogue != BP_GEMM_EPILOGUE_NONE ? &dummy : nullptr)) return BP_ERR_GEMM;
    hipblasLtMatmulPreference_t pref = nullptr;
    if (l.pref_create(&pref) != HIPBLAS_STATUS_SUCCESS) return BP_ERR_GEMM;
    const uint64_t ws = kWorkspaceBytes;
    std::vector<hipblasLtMatmulHeuristicResult_t> found;
    found.resize(static_cast<size_t>(max_solutions));
    int n = 0;
    const bool ok = l.pref_set(pref, HIPBLASLT_MATMUL_PREF_MAX_WORKSPACE_BYTES, &ws, sizeof(ws)) == HIPBLAS_STATUS_SUCCESS
        && l.heuristic(dev.handle, p.desc, p.w, p.a, p.d, p.d, pref, max_solutions, found.data(), &n) == HIPBLAS_STATUS_SUCCESS;
    l.pref_destroy(pref);
    if (!ok) return BP_ERR_GEMM;
    for (int i = 0; i < n && i < max_solutions; ++i)
        if (found[size_t(i)].state == HIPBLAS_STATUS_SUCCESS) solutions[(*count)++] = l.index_from_algo(found[size_t(i)].algo);
    return BP_OK;
}

}  // extern "C"
