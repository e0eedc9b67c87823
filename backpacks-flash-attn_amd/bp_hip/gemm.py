"""Dense layers by a pinned hipBLASLt solution (C ABI bp_gemm_bf16 / bp_gemm_f16, csrc/bp_gemm.hip).

`linear(x, w, bias, gelu, out)` is what the inference paths call for x W^T (+ b) (-> tanh-GELU).  A table
(bp_hip/gemm_solutions.json, written by scripts/tune_gemm.py from measurements on the device) names, for a few large
shapes, the library solution that was measured to beat the heuristic's pick by more than that pick's own spread.  A
call whose (dtype, epilogue, N, K) has a row with m_min <= M runs exactly that solution; every other call -- any shape
below 131 072 rows among them, so decoding and every small model -- runs the torch call it ran before, bit for bit.
Which algorithm runs is a function of the table alone: nothing is tuned at run time."""
import contextlib
import ctypes
import json
import os
import warnings

import torch
import torch.nn.functional as F

EPILOGUES = ('none', 'bias', 'bias_gelu')            # BP_GEMM_EPILOGUE_*
DTYPES = {'fp16': torch.float16, 'bf16': torch.bfloat16}
_DTYPE_CODES = {torch.float16: 0, torch.bfloat16: 1}
M_BUCKET_MIN = 131072     # no row of the SHIPPED table may apply below this many rows (tests/test_gemm_table.py)
STATUS = {0: 'ran', 1: 'miss', 2: 'version', 3: 'unsupported', 4: 'capturing', 5: 'no_library'}    # BP_GEMM_*
TABLE_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'gemm_solutions.json')


class GemmRow(ctypes.Structure):
    """bp_gemm_row of include/bp_hip.h."""
    _fields_ = [('dtype', ctypes.c_int32), ('epilogue', ctypes.c_int32), ('n', ctypes.c_int32), ('k', ctypes.c_int32),
                ('m_min', ctypes.c_int64), ('version', ctypes.c_int32), ('solution', ctypes.c_int32),
                ('arch', ctypes.c_char * 16)]


class GemmTable:
    """A parsed solutions table.  `spec`: the dict of gemm_solutions.json --
        {'library_version': int, 'arch': 'gfx950', 'entries': [row, ...], 'lm_head_chunk_rows': {'<M>': rows}}
    with row = {'dtype': 'bf16' | 'fp16', 'epilogue': 'none' | 'bias' | 'bias_gelu', 'n', 'k', 'm_min', 'solution'
    (None: keep the heuristic), optionally 'library_version' / 'arch' of its own, and the measurement it came from}."""

    def __init__(self, spec):
        self.spec = spec
        self.library_version = int(spec.get('library_version', 0))
        self.arch = str(spec.get('arch', ''))
        rows = []
        for e in spec.get('entries', ()):
            if e.get('solution') is None:
                continue                  # "keep the heuristic": recorded for the reader, no row for the library
            arch = str(e.get('arch', self.arch)).encode()
            if len(arch) > 15:
                raise ValueError(f'gemm table: arch string too long: {arch!r}')
            if int(e['m_min']) < 1:
                raise ValueError('gemm table: m_min must be >= 1')
            rows.append(GemmRow(_DTYPE_CODES[DTYPES[e['dtype']]], EPILOGUES.index(e['epilogue']), int(e['n']), int(e['k']),
                                int(e['m_min']), int(e.get('library_version', self.library_version)), int(e['solution']), arch))
        self.n_rows = len(rows)
        self.rows = (GemmRow * max(1, self.n_rows))(*rows)
        # smallest m_min per (dtype code, epilogue, n, k): the host-side filter that keeps every other call off the library
        self.floor = {}
        for r in rows:
            key = (r.dtype, r.epilogue, r.n, r.k)
            self.floor[key] = min(self.floor.get(key, r.m_min), r.m_min)
        self.chunk_rows = {int(m): int(c) for m, c in (spec.get('lm_head_chunk_rows') or {}).items()}

    @classmethod
    def load(cls, path=TABLE_PATH):
        if not os.path.exists(path):
            return cls({})
        with open(path) as f:
            return cls(json.load(f))


_shipped = None
_library_here = None    # library() of this process, once asked
_refusal_said = []      # the status of the one 'version' / 'no_library' refusal that was warned about


def shipped_table():
    global _shipped
    if _shipped is None:
        _shipped = GemmTable.load()
    return _shipped


@contextlib.contextmanager
def use_table(table):
    """Within the block, `table` stands in for the shipped one in every call that names none (tests, the tuning tool)."""
    global _shipped
    previous, _shipped = shipped_table(), table
    try:
        yield table
    finally:
        _shipped = previous


def library():
    """(hipblasLtGetVersion, arch) of the libhipblaslt this process has loaded, as table rows state them."""
    import bp_hip
    version, arch = ctypes.c_int(0), ctypes.create_string_buffer(32)
    code = bp_hip.lib().bp_gemm_library(ctypes.byref(version), arch, 32)
    if code != 0:
        raise RuntimeError(f'bp_gemm_library: status {code} ({STATUS.get(code) or bp_hip.lib().bp_strerror(code).decode()})')
    return version.value, arch.value.decode()


def heuristic(dtype, epilogue, m, n, k, lda=None, ldw=None, ldd=None, count=32):
    """Solution indices of the library heuristic's first `count` candidates for a problem, best first."""
    import bp_hip
    sol, got = (ctypes.c_int * count)(), ctypes.c_int(0)
    code = bp_hip.lib().bp_gemm_heuristic(_DTYPE_CODES[dtype], EPILOGUES.index(epilogue), m, n, k, lda or k, ldw or k,
                                          ldd or n, sol, count, ctypes.byref(got))
    if code != 0:
        raise RuntimeError(f'bp_gemm_heuristic: status {code} ({STATUS.get(code) or bp_hip.lib().bp_strerror(code).decode()})')
    return list(sol[:got.value])


def pinned(x2, w, bias, gelu, out2, table):
    """Run the GEMM of 2-D operands by `table`'s solution into out2.  Returns the BP_GEMM_* status name: 'ran', or why
    nothing was launched.  A library error raises."""
    import bp_hip
    epilogue = 0 if bias is None else (2 if gelu else 1)
    m, k = x2.shape
    n = w.shape[0]
    floor = table.floor.get((_DTYPE_CODES[x2.dtype], epilogue, n, k))
    if floor is None or m < floor:
        return 'miss'
    fn = bp_hip.lib().bp_gemm_bf16 if x2.dtype == torch.bfloat16 else bp_hip.lib().bp_gemm_f16
    with torch.cuda.device(x2.device):
        code = fn(x2.data_ptr(), w.data_ptr(), bias.data_ptr() if bias is not None else None, out2.data_ptr(),
                  m, n, k, x2.stride(0), w.stride(0), out2.stride(0), epilogue, table.rows, table.n_rows, None,
                  ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    if code < 0:
        raise RuntimeError(f'bp_gemm failed: {bp_hip.lib().bp_strerror(code).decode()} (code {code})')
    if code in (2, 5) and not _refusal_said:
        # the whole table is then dead weight: say so once, or the gain it was measured for disappears in silence
        _refusal_said.append(code)
        warnings.warn('bp_hip.linear: the table of pinned hipBLASLt solutions is not used -- ' + (
            f'it was measured with library version {table.library_version} on {table.arch!r}, not the ones in this process; '
            'run scripts/tune_gemm.py again' if code == 2 else
            'no libhipblaslt with the expected entry points is loaded in this process') + '.  Every GEMM takes the torch call.')
    return STATUS[code]


def _rows_ok(t):
    return t.dim() == 2 and t.stride(1) == 1 and t.stride(0) >= t.shape[1]


def linear(x, w, bias=None, gelu=False, out=None, table=None):
    """x (..., K) W(N, K)^T (+ bias (N,)) (-> tanh-GELU when `gelu`; needs a bias) -> (..., N), or into `out` (M, N) rows
    of a caller-owned buffer.  Under no_grad, on 16-bit CUDA tensors, a row of `table` (default: the shipped one) that
    applies runs its pinned solution; otherwise the call is torch's, as before this helper existed."""
    table = shipped_table() if table is None else table
    if (table.n_rows and not torch.is_grad_enabled() and x.is_cuda and x.dtype in _DTYPE_CODES and w.dtype == x.dtype
            and (bias is None or bias.dtype == x.dtype) and (bias is not None or not gelu) and x.numel() > 0
            and w.dim() == 2 and w.is_cuda and (bias is None or (bias.is_cuda and bias.is_contiguous()))):
        x2 = x.reshape(-1, x.shape[-1]) if x.is_contiguous() else x
        if _rows_ok(x2) and _rows_ok(w) and (out is None or (_rows_ok(out) and out.dtype == x.dtype
                                                               and out.shape == (x2.shape[0], w.shape[0]))):
            m, n = x2.shape[0], w.shape[0]
            floor = table.floor.get((_DTYPE_CODES[x.dtype], 0 if bias is None else (2 if gelu else 1), n, x2.shape[1]))
            # (a stream under capture keeps torch's GEMM: nothing is allocated for a call the entry would refuse)
            if floor is not None and m >= floor and not torch.cuda.is_current_stream_capturing():
                o2 = out if out is not None else torch.empty((m, n), dtype=x.dtype, device=x.device)
                if pinned(x2, w, bias, gelu, o2, table) == 'ran':
                    return o2 if out is not None else o2.view(*x.shape[:-1], n)
    if out is not None:
        x2 = x.reshape(-1, x.shape[-1])
        if gelu:
            raise RuntimeError('bp_hip.linear: out= with gelu is not a call the models make')
        return torch.mm(x2, w.t(), out=out) if bias is None else torch.addmm(bias, x2, w.t(), out=out)
    if gelu:
        return torch._addmm_activation(bias, x.reshape(-1, x.shape[-1]), w.t(), use_gelu=True).view(*x.shape[:-1], w.shape[0])
    return F.linear(x, w, bias)


def lm_head_chunk_rows(m, table=None):
    """Row chunk the LM head's GEMM of `m` rows should be cut into by the table's measurement (0: one GEMM)."""
    table = shipped_table() if table is None else table
    rows = table.chunk_rows.get(int(m), 0) if table.n_rows else 0
    if rows:
        # the measurement holds for the library and the device it was taken with, like the rows themselves
        global _library_here
        if _library_here is None:
            try:
                _library_here = library()
            except RuntimeError:
                _library_here = (None, None)
        if _library_here != (table.library_version, table.arch):
            return 0
    return rows
