// Ring format and job protocol of the persistent sense-mix kernels: sense_mix_dma_kernel (sense_mix_dma.hip, the forward)
// and sense_mix_dc_kernel (sense_mix_bwd.hip, dC -- the forward with the roles of queries and keys exchanged).
//
// Both own 256 rows x 256 output columns of one sample per job (8 waves x 32 rows: one row per lane, its 16-column
// fragments and the accumulators in registers) and stream 64-row tiles of the OTHER side through a 3-slot LDS-DMA ring:
//   * operand A -- 16-bit rows of d_k columns, the A operand of the score MFMAs (K in the forward, Q in dC): AROW bytes
//     per row (128 or 256), 16-byte slots XOR-swizzled (k_swz, bp_dma.h);
//   * operand B -- 256 output columns per row, read TRANSPOSED as the A operand of the accumulating MFMAs (C in the
//     forward, dout in dC): 512-byte rows, 64-byte chunks XOR-swizzled (v_lds_off<8>, bp_common.h);
//   * optionally 64 fp32 aux words per wave (the tile's key weights in the weighted forward, the log-sum-exp of its
//     queries in dC): every wave fetches its own copy into its own 256-byte slot;
//   * behind the three stages the 16-byte job word.
// The swizzles are applied to the per-lane SOURCE address of the DMA pieces; every wave issues DMA_PER_STAGE pieces per
// tile, which is what the counted waits rely on (bp_dma.h).  What differs between the kernels -- masks, liveness, the
// order of clean and diagonal steps, where the accumulators go -- stays in their files.
#pragma once
#include "bp_common.h"
#include "bp_dma.h"
#include "bp_kernels.h"

namespace bp {

template <int KD_, bool AUX_>
struct MixRingCfg {
    static constexpr int KD = KD_;
    static constexpr bool AUX = AUX_;
    static constexpr int BM = 256, BK = 64, NB = 8, BNC = 256, NT = 512, NWAVE = 8, NSTAGE = 3;
    static constexpr int AROW = KD <= 4 ? 128 : 256;   // bytes per A row (power of two, XOR-swizzled)
    static constexpr int ASLOTS = AROW / 16;
    static constexpr int BROW = 512;                    // bytes per B row (256 columns)
    static constexpr int ATILE = BK * AROW;
    static constexpr int BTILE = BK * BROW;
    static constexpr int AUX_OFF = ATILE + BTILE;
    static constexpr int XTILE = AUX ? NWAVE * 256 : 0;   // per wave: 64 fp32 aux words of the tile
    static constexpr int STAGE = ATILE + BTILE + XTILE;
    static constexpr int A_DMA = ATILE / 1024 / NWAVE;   // DMA instructions per wave per tile (1 or 2)
    static constexpr int B_DMA = BTILE / 1024 / NWAVE;   // 4
    static constexpr int DMA_PER_STAGE = A_DMA + B_DMA + (AUX ? 1 : 0);
    static constexpr uint32_t ALL_PIECES = (1u << DMA_PER_STAGE) - 1u;   // bit j: A pieces, then B pieces, then the aux piece
    static constexpr int A_ROWS_PER_DMA = 1024 / AROW;   // 8 or 4
    static constexpr int JOB_OFF = NSTAGE * STAGE;       // 16 bytes: job broadcast
    static constexpr int SMEM = JOB_OFF + 16;
    static_assert(NB == 8, "the B read offsets assume 8 column blocks");
};

// ---- job protocol ----------------------------------------------------------------------------------------------------
// A job = (group, tile): a group is a (sample, column chunk) pair, a tile 256 rows.  One ticket counter per XCD
// (MixQueues, armed in front of the launch); tickets of a queue run through ALL its groups' tiles of rank 0, then rank 1,
// ...; the kernel decides which tile has which rank (heaviest first).  A workgroup whose own queue is empty steals from
// the others.  The job word is group * kMixMaxTiles + rank, -1 when nothing is left.
struct MixJob {
    int batch, col_base, rank;
};

// thread 0 only
BP_DEV int mix_next_job(MixQueues *queues, uint32_t &exhausted, int b, int n_chunks, int n_tiles) {
    const int my_xcd = blockIdx.x & 7;
    for (int t = 0; t < 8; ++t) {
        const int q = (my_xcd + t) & 7;
        if (exhausted & (1u << q)) continue;
        const int groups = mix_queue_groups(b, n_chunks, q);
        const int njobs = groups * n_tiles;
        const int idx = njobs > 0 ? (int)atomicAdd(&queues->ticket[q], 1u) : njobs;
        if (idx < njobs) {
            // all groups' heaviest tiles first (a group's tiles together, so that its C slab is re-read while it might
            // still be cached, gained nothing: 1.32 / 1.34 ms against 1.29 / 1.28 ms at B = 64, same fetch traffic, r02_e)
            // (sample-major order -- one sample's twelve jobs together -- fetches 4 % less and runs 2-3 % slower, r02_w)
            // (table form, r04_ab: walking the queue column chunk by column chunk, so that the rows in flight chip-wide are
            // one chunk's third of the table, is 1-2 % slower at B = 64 ... 2048 -- the memory-side cache does not pay it back)
            // (a group's query tiles as consecutive tickets, profiles/r06_c_ab_mix_order_4096.jsonl, and paired tickets,
            // profiles/r06_t_ab_mix_paired_tickets_*.txt, were measured and not adopted)
            const int rank = idx / groups;
            const int grp = mix_queue_group(n_chunks, q, idx - rank * groups);
            return grp * kMixMaxTiles + rank;
        }
        exhausted |= 1u << q;
    }
    return -1;
}

// Whole workgroup: fetch the next job and broadcast it through the job word; returns the word.  `exhausted` (bit q: queue
// q has no jobs left) lives across the kernel's job loop; only thread 0 uses it.
// (The word is returned and decoded by a second call on purpose: with the end test and the decode inside this function
// every instantiation spilled three to five more scalar registers, and the forward's d_k = 128 one more vector register.)
template <class C> BP_DEV int mix_take_job(char *smem, MixQueues *queues, uint32_t &exhausted, int b, int n_chunks, int n_tiles) {
    __syncthreads();   // every wave is done with the previous job's ring (and has read its job word)
    if (threadIdx.x == 0) *reinterpret_cast<int *>(smem + C::JOB_OFF) = mix_next_job(queues, exhausted, b, n_chunks, n_tiles);
    __syncthreads();
    return __builtin_amdgcn_readfirstlane(*reinterpret_cast<const int *>(smem + C::JOB_OFF));
}
// a job word >= 0 -> the job
template <class C> BP_DEV MixJob mix_decode_job(int word, int n_chunks) {
    const int grp = word / kMixMaxTiles;
    const int batch = grp / n_chunks;
    return MixJob{batch, (grp - batch * n_chunks) * C::BNC, word % kMixMaxTiles};
}

// ---- reading a tile --------------------------------------------------------------------------------------------------
// lane-constant LDS read offsets of the two operands.  The LDS array itself is an argument of every read, not a member:
// as a member of this struct the pointer cost dC's d_k <= 32 instantiations one register.
template <class C> struct MixTileReader {
    int a_off[C::KD];   // A fragment: row l31 (+32*kk), logical slot 2*s + hh
    int b_off[4];       // B^T fragment, see below

    BP_DEV MixTileReader(int lane) {
        const int l31 = lane & 31, hh = lane >> 5;
#pragma unroll
        for (int s = 0; s < C::KD; ++s) a_off[s] = RowImage<C::AROW>::read_off(l31, hh, s);
        // (k_swz only looks at row bits 0..3, so +32 rows keeps the same swizzle)
        const int row_lane = 4 * hh + ((lane & 15) >> 2);
        const int ch_lane = ((lane >> 4) & 1) * 2 + ((lane & 3) >> 1);
        // B^T fragment: (row row_lane, 16-col group of block n), +8 rows keeps swizzle.  The swizzle XORs the 64-B chunk
        // index n with row & 3, i.e. only its low two bits: block n + 4 sits exactly 256 bytes after block n, so four
        // lane offsets + an immediate serve the eight blocks.
#pragma unroll
        for (int n = 0; n < 4; ++n) b_off[n] = v_lds_off<C::NB>(row_lane, n * 4 + ch_lane) + (lane & 1) * 8;
    }
    // A operand of column step s, 32-row half kk of the tile at ring byte offset `stage`
    BP_DEV u32x4 a_operand(const char *smem, int stage, int s, int kk) const { return lds_read_16B(smem, a_off[s] + stage + kk * 32 * C::AROW); }
    // B^T operand of column block n at LDS byte offset `rows` (16 rows x 256 columns)
    BP_DEV u32x4 b_operand(const char *smem, int rows, int n) const { return tr_operand(smem, b_off[n & 3] + (n >> 2) * 256 + rows, C::BROW); }
};

// scores of the 32-row half kk of the tile at `stage` against my fragments `frag`: tile rows along the registers
template <class E, class C> BP_DEV f32x16 mix_scores(const char *smem, const MixTileReader<C> &rd, int stage, int kk, const u32x4 (&frag)[C::KD]) {
    f32x16 st;
#pragma unroll
    for (int r = 0; r < 16; ++r) st[r] = 0.f;
#pragma unroll
    for (int s = 0; s < C::KD; ++s) st = E::mfma(rd.a_operand(smem, stage, s, kk), frag[s], st);
    return st;
}
// ... of both halves as one operand stream, alternating accumulators (the per-half form waits for an LDS round trip in
// front of each of its KD dependent MFMAs: ~600 clocks for the six of d_k = 48)
template <class E, class C>
BP_DEV void mix_scores_both(const char *smem, const MixTileReader<C> &rd, int stage, const u32x4 (&frag)[C::KD], f32x16 &st0, f32x16 &st1) {
#pragma unroll
    for (int r = 0; r < 16; ++r) st0[r] = st1[r] = 0.f;
    mfma_stream<2 * C::KD>([&](int i) { return rd.a_operand(smem, stage, i >> 1, i & 1); },
                           [&](int i, const u32x4 &a) {
                               if (i & 1) { st1 = E::mfma(a, frag[i >> 1], st1); asm volatile("" : "+v"(st1)); }
                               else { st0 = E::mfma(a, frag[i >> 1], st0); asm volatile("" : "+v"(st0)); }
                           });
}
// probabilities of a half -> the two B operands (16 tile rows each) of the accumulating MFMAs
template <class E> BP_DEV void mix_pack(const f32x16 &st, u32x4 (&pf)[2]) {
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int i = 0; i < 4; ++i) pf[ks][i] = E::pack2(st[ks * 8 + 2 * i], st[ks * 8 + 2 * i + 1]);
}
// acc^T += B^T P over NP consecutive 16-row steps (pk[0..NP-1]) from row `row0` of the tile at `stage`: 8 NP MFMAs as ONE
// operand stream with the B^T operand of MFMA i + 2 requested before MFMA i issues (mfma_stream, bp_common.h) -- hipcc
// on its own puts "2 ds_read, s_waitcnt lgkmcnt(0)" in front of every MFMA: 75-85 clocks per MFMA where the pipe needs 32
// (r03_aa/ab timelines).  `mid(i)` runs behind MFMA i (DMA issue points).  Column blocks from nb_live on are never stored.
template <class E, class C, bool FULL, int NP, class Mid>
BP_DEV void mix_pv_stream(const char *smem, const MixTileReader<C> &rd, f32x16 (&acc)[C::NB], int nb_live, int stage, int row0,
                          const u32x4 (&pk)[NP], Mid &&mid) {
    const int base = stage + C::ATILE + row0 * C::BROW;
    mfma_stream<NP * C::NB>([&](int i) { return rd.b_operand(smem, base + (i >> 3) * 16 * C::BROW, i & 7); },
                            [&](int i, const u32x4 &a) {
                                if (FULL || (i & 7) < nb_live) acc[i & 7] = E::mfma(a, pk[i >> 3], acc[i & 7]);
                                asm volatile("" : "+v"(acc[i & 7]));
                                mid(i);
                            });
}
// The 8 MFMAs of half 0, rows 0..15 (`p0`), each followed by 2 fma + 2 exp of half 1 (`st1`: scores in, probabilities out;
// `lse2(r)` = log-sum-exp in log2 units that belongs to register r); the B^T operand of MFMA n+1 is requested before
// MFMA n issues, so the LDS latency hides behind a full MFMA
template <class E, class C, bool FULL, class Lse>
BP_DEV void mix_x_block(const char *smem, const MixTileReader<C> &rd, f32x16 (&acc)[C::NB], int nb_live, int stage, const u32x4 &p0,
                        f32x16 &st1, float c2, Lse &&lse2) {
    const int rows = stage + C::ATILE;
    u32x4 a = rd.b_operand(smem, rows, 0);
#pragma unroll
    for (int n = 0; n < C::NB; ++n) {
        u32x4 a_next = a;
        if (n + 1 < C::NB) a_next = rd.b_operand(smem, rows, n + 1);
        asm volatile("" : "+v"(a));
        if (FULL || n < nb_live) acc[n] = E::mfma(a, p0, acc[n]);   // (partial last column chunk: d = 640, 384, ...)
        asm volatile("" : "+v"(acc[n]));
        float x0 = st1[2 * n], x1 = st1[2 * n + 1];
        asm volatile("" : "+v"(x0), "+v"(x1));
        x0 = fast_exp2(fmaf(x0, c2, -lse2(2 * n)));
        x1 = fast_exp2(fmaf(x1, c2, -lse2(2 * n + 1)));
        asm volatile("" : "+v"(x0), "+v"(x1));
        st1[2 * n] = x0;
        st1[2 * n + 1] = x1;
        a = a_next;
    }
}
// my row's 256 accumulated columns as 16-bit 8-byte stores to `row` (column col_base of it), columns < ncols only
// (plain stores: 8-byte per-lane pieces marked non-temporal cost 1.6 -> 4.6 ms in dC, r02_p)
template <class E, class C> BP_DEV void mix_store_row(uint16_t *row, const f32x16 (&acc)[C::NB], int col_base, int ncols, int hh) {
#pragma unroll
    for (int n = 0; n < C::NB; ++n)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int col = col_base + n * 32 + 8 * g + 4 * hh;
            if (col < ncols) {
                u32x2 w = {E::pack2(acc[n][4 * g + 0], acc[n][4 * g + 1]), E::pack2(acc[n][4 * g + 2], acc[n][4 * g + 3])};
                *reinterpret_cast<u32x2 *>(row + col) = w;
            }
        }
}

// ---- filling the ring ------------------------------------------------------------------------------------------------
// The DMA side of one job: tiles [t_begin, t_end) of every sense in turn, two tiles in flight.  A step past the end
// re-fetches the last tile (harmless, keeps every wave's DMA count per step constant so the counted wait never changes).
//
// Per-lane byte offsets of my DMA pieces inside a tile (the scalar tile base is added by the DMA instruction; the piece rows
// and tr_lane stay spelled here: RowImage / TrImage::src on the opaque lane copy changed the generated code).  A piece
// j of this wave: rows (wave*A_DMA + j)*A_ROWS_PER_DMA + lane/ASLOTS, stored slot lane%ASLOTS; B piece j: rows
// (wave*B_DMA + j)*2 + lane/32, stored chunk lane%32.  They are rebuilt PER JOB from an opaque copy of the lane
// index: as loop invariants hipcc hoists the row / column tables to kernel entry and keeps them alive across
// the whole job loop -- ten registers that the d_k = 48 instantiation then spilled to scratch (round-3 review).
// The job's only possible partial tile (the last one, when the sequence ends inside it) clamps its rows to the
// final valid row inside issue(), in a cold branch, instead of carrying a second offset set.
//
// The base pointers at2 / bt2 of the tile two steps ahead are carried and advanced on the scalar unit once per step
// (advance2): recomputing them from (sense, tile) in each of a step's calls cost ~120 SALU instructions per step.
template <class C> struct MixStream {
    uint32_t lds0;
    int wave, lane, lane_o, S;
    int nsenses, t_begin, t_end;
    int t_partial, last_row;
    int l2, t2;                  // (sense, tile) of step + 2
    const uint16_t *as2, *bs2;   // first tile of sense l2
    const uint16_t *at2, *bt2;   // ... tile t2 of it
    int64_t a_rs, a_ss, a_tile_step, b_ss, b_tile_step;
    uint32_t a_voff[C::A_DMA];
    int slot;                    // ring slot of the current step

    BP_DEV int a_piece_row(int j) const { return (wave * C::A_DMA + j) * C::A_ROWS_PER_DMA + lane_o / C::ASLOTS; }
    BP_DEV int b_piece_row(int j) const { return (wave * C::B_DMA + j) * 2 + (lane_o >> 5); }

    // a / b: the sample's operands (sense 0, row 0), row / sense strides in elements (b_ss = 0: B is the same for every
    // sense); the job's tiles start at t_begin and end with the one that holds row rows_end - 1
    BP_DEV void begin_job(uint32_t lds0_, int wave_, int lane_, int S_, int nsenses_, int t_begin_, int rows_end,
                          const uint16_t *a, int64_t a_rs_, int64_t a_ss_, int dk, const uint16_t *b, int64_t b_rs, int64_t b_ss_) {
        lds0 = lds0_, wave = wave_, lane = lane_, S = S_, nsenses = nsenses_, t_begin = t_begin_;
        a_rs = a_rs_, a_ss = a_ss_, b_ss = b_ss_;
        t_end = (rows_end + C::BK - 1) / C::BK;
        lane_o = lane;
        asm volatile("" : "+v"(lane_o));
        t_partial = (rows_end == S && (S % C::BK) != 0) ? t_end - 1 : -1;
        last_row = S - 1 - (t_end - 1) * C::BK;
#pragma unroll
        for (int j = 0; j < C::A_DMA; ++j) {
            const int row = a_piece_row(j);
            const int logical = (lane_o % C::ASLOTS) ^ k_swz<C::AROW>(row);
            const int col = logical * 8 < dk ? logical * 8 : 0;   // pad slot: a duplicate of column 0 (finite; meets zero columns)
            a_voff[j] = (uint32_t)(row * a_rs + col) * 2u;
        }
        l2 = 0, t2 = t_begin;
        a_tile_step = (int64_t)C::BK * a_rs, b_tile_step = (int64_t)C::BK * b_rs;
        as2 = at2 = a + (int64_t)t_begin * a_tile_step;
        bs2 = bt2 = b + (int64_t)t_begin * b_tile_step;
    }
    // offsets of my B pieces: rows with stride row_stride (0: the caller adds the row itself), 16-byte chunks of the 256
    // columns from col_base; chunks at or past ncols receive a duplicate of column col_base (never stored)
    template <bool FULL> BP_DEV void b_offsets(uint32_t (&b_voff)[C::B_DMA], int64_t row_stride, int col_base, int ncols) const {
#pragma unroll
        for (int j = 0; j < C::B_DMA; ++j) {
            const int row = b_piece_row(j);
            const int logical = TrImage<C::NB>::flip(row, lane_o & 31);   // stored chunk -> logical chunk
            const int col = (FULL || col_base + logical * 8 < ncols) ? col_base + logical * 8 : col_base;
            b_voff[j] = (uint32_t)(row * row_stride + col) * 2u;
        }
    }

    // DMA pieces of the tile two steps ahead into ring slot `to_slot`; `pieces` selects a subset (C::ALL_PIECES bits).
    // b_piece(j, back, lds_dst) issues B piece j with its rows moved `back` rows up (partial tile: onto the last valid
    // row); aux_row(l) -> the fp32 row of sense l whose element t holds the aux word of tile row t.
    template <class BPiece, class AuxRow> BP_DEV void issue(int to_slot, uint32_t pieces, BPiece &&b_piece, AuxRow &&aux_row) const {
        const uint32_t stage_off = lds0 + to_slot * C::STAGE;
        if (__builtin_expect(t2 == t_partial, 0)) {
#pragma unroll
            for (int j = 0; j < C::A_DMA; ++j)
                if ((pieces >> j) & 1u) {
                    const uint32_t back = (uint32_t)(max(a_piece_row(j) - last_row, 0) * a_rs) * 2u;
                    dma16_s(at2, a_voff[j] - back, __builtin_amdgcn_readfirstlane(stage_off + (wave * C::A_DMA + j) * 1024));
                }
#pragma unroll
            for (int j = 0; j < C::B_DMA; ++j)
                if ((pieces >> (C::A_DMA + j)) & 1u)
                    b_piece(j, max(b_piece_row(j) - last_row, 0),
                            __builtin_amdgcn_readfirstlane(stage_off + C::ATILE + (wave * C::B_DMA + j) * 1024));
        } else {
#pragma unroll
            for (int j = 0; j < C::A_DMA; ++j)
                if ((pieces >> j) & 1u) dma16_s(at2, a_voff[j], stage_off + (wave * C::A_DMA + j) * 1024);
#pragma unroll
            for (int j = 0; j < C::B_DMA; ++j)
                if ((pieces >> (C::A_DMA + j)) & 1u) b_piece(j, 0, stage_off + C::ATILE + (wave * C::B_DMA + j) * 1024);
        }
        if (C::AUX && ((pieces >> (C::A_DMA + C::B_DMA)) & 1u)) {
            // aux words of this (sense, tile): lane i fetches the word of tile row i into the wave's own 256-B slot
            dma4(aux_row(l2) + min(t2 * C::BK + lane, S - 1), stage_off + C::AUX_OFF + wave * 256);
        }
    }
    BP_DEV void advance2() {
        if (t2 + 1 < t_end) {
            ++t2;
            at2 += a_tile_step;
            bt2 += b_tile_step;
        } else if (l2 + 1 < nsenses) {
            ++l2;
            t2 = t_begin;
            as2 += a_ss;
            bs2 += b_ss;
            at2 = as2;
            bt2 = bs2;
        }
    }
    // the first two tiles; issue_all(slot) = issue(slot, C::ALL_PIECES, ...) with the kernel's pieces
    template <class Issue> BP_DEV void prime(Issue &&issue_all) {
        issue_all(0);
        advance2();
        issue_all(1);
        advance2();
        slot = 0;
    }
    BP_DEV static void step_begin() {
        wait_vmcnt<C::DMA_PER_STAGE>();   // my share of the current tile has landed (the next may be in flight)
        __builtin_amdgcn_s_barrier();     // ... and everybody's; all waves are done reading slot (slot + 2) % 3
    }
    BP_DEV void step_end() {
        slot = slot == 2 ? 0 : slot + 1;
        advance2();
    }
    BP_DEV int stage() const { return slot * C::STAGE; }          // byte offset of the current step's tile
    BP_DEV int refill_slot() const { return slot >= 1 ? slot - 1 : 2; }   // where tile + 2 goes: the slot read last step
};

// ---- host side -------------------------------------------------------------------------------------------------------
// A persistent launch: arm the queue record, one workgroup per CU (or per job), dispatch on dtype / KD / FULL.
// launch(et, kd, full, grid, block, p) enqueues the kernel.  Requires n_tiles <= kMixMaxTiles.
template <class Params, class Launch>
hipError_t launch_mix_persistent(const Params &params, int n_tiles, int ncols, int dtype, hipStream_t stream, Launch &&launch) {
    Params p = params;
    const hipError_t armed = arm_mix_queues(p.queues, stream);
    if (armed != hipSuccess) return armed;
    const dim3 g(persistent_grid(p.b * p.n_chunks * n_tiles)), t(512);   // >= 120 KB of LDS: one workgroup per CU
    return with_dtype(dtype, [&](auto et) {
        return with_kd(p.dk, [&](auto kd) {
            return with_flag(ncols % 256 == 0, [&](auto full) {
                launch(et, kd, full, g, t, p);
                return hipGetLastError();
            });
        });
    });
}

}  // namespace bp
