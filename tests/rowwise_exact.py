"""Exact-ownership inputs for the row-wise kernels (csrc/add_layer_norm.hip, bias_gelu.hip, xentropy.hip, softmax_bwd.hip):
tests/test_gpu_rowwise_exact.py and its CPU pre-check tests/test_rowwise_exact_host.py share the builders, the case lists, the
expected results and the criteria below -- what tests/prefill_needles.py is for the attention kernels.

The inputs are small integers and powers of two, a fixed hash of their indices (no generator state, any device), chosen so
that every fp32 intermediate of the kernel is exact (partial sums stay below 2^24): the fp64 result rounded ONCE to the output
dtype is then the only right answer, and one row or column that is lost, counted twice or taken from a neighbour changes
bits.  Where a kernel's own arithmetic cannot be exact (the LayerNorm statistics, label smoothing) the criterion is a bound
that comes from an fp32 evaluation of the same formulas on the CPU, never from the kernel.

Every output of a call is a view inside a larger NaN-filled buffer (`Guarded`): at least one row of guard before and after
it, and the gap columns where a row stride exceeds the width.  The guard must hold the same bits afterwards.

The tiling constants the cases aim at are computed, not assumed: `unrolled_trips` (bias_gelu_bwd_kernel's U-unrolled main
loop and its tail, from the slice count the library reports), `ln_bwd_trips` (the grid-stride loop of the LayerNorm backward,
from the workgroup cap the library reports), `xent_split` (head / vector body / tail of a cross-entropy row, from its address).
"""
import torch

NAN = float('nan')
LOG2E = 1.4426950408889634
LN2 = 0.6931471805599453
BITS = {torch.bfloat16: torch.int16, torch.float16: torch.int16, torch.float32: torch.int32}
MANT = {torch.bfloat16: 7, torch.float16: 10, torch.float32: 23}             # stored mantissa bits
MIN_EXP = {torch.bfloat16: -126, torch.float16: -14, torch.float32: -126}    # exponent of the smallest normal number
ROUNDING = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11, torch.float32: 2.0 ** -24}
DTYPE_CODE = {torch.float16: 0, torch.bfloat16: 1, torch.float32: 2}         # BP_DTYPE_*
EPS = 1e-5


def _hash(ids):
    x = (ids.long() * 2654435761 + 40503) & 0xffffffff
    x = ((x ^ (x >> 15)) * 2246822519) & 0xffffffff
    return x ^ (x >> 13)


def rc_hash(rows, cols, device, salt=0):
    """(rows, cols) int64 hash of (row, column, salt)."""
    r = torch.arange(rows, device=device)[:, None]
    c = torch.arange(cols, device=device)[None, :]
    return _hash(r * 16411 + c + salt * 1000003)


def round_once(x64, dtype):
    """fp64 -> dtype with ONE rounding: the value must be an fp32 number (checked), which torch then rounds to 16 bit."""
    x32 = x64.float()
    assert torch.equal(x32.double(), x64), 'expected value is not exact in fp32'
    return x32.to(dtype)


def ulp(x64, dtype):
    """Spacing of `dtype` at |x| (fp64 tensor); the subnormal spacing below the smallest normal number."""
    e = torch.floor(torch.log2(x64.abs().clamp(min=2.0 ** MIN_EXP[dtype])))
    return torch.exp2(e - MANT[dtype])


def listing(bad, what, limit=4):
    """Failure lines for the positions where the boolean tensor `bad` is set."""
    n = int(bad.sum())
    if n == 0:
        return []
    where = bad.nonzero()[:limit].tolist()
    return [f'{what}: {n} wrong, first at {where}']


# ---- guarded buffers -------------------------------------------------------------------------------------------------------

class Guarded:
    """A (rows, cols) view with row stride `stride` (elements) that starts `offset` elements behind a 16-byte boundary, inside
    a flat NaN buffer with at least one row of guard on either side."""

    def __init__(self, rows, cols, dtype, device, stride=None, offset=0):
        stride = stride or cols
        assert stride >= cols
        per16 = 16 // torch.empty(0, dtype=dtype).element_size()
        guard = -(-max(stride, 1) // per16) * per16
        self.buf = torch.full((guard + offset + rows * stride + guard + per16,), NAN, dtype=dtype, device=device)
        assert self.buf.data_ptr() % 16 == 0
        self.geometry = ((rows, cols), (stride, 1), guard + offset)
        self.view = self.buf.as_strided(*self.geometry)
        self.nan_bits = torch.full((1,), NAN, dtype=dtype).view(BITS[dtype]).item()

    def ptr(self):
        return self.view.data_ptr()

    def failures(self, what):
        """Guard rows and gap columns must hold the bits they were given."""
        outside = torch.ones(self.buf.numel(), dtype=torch.bool, device=self.buf.device)
        outside.as_strided(*self.geometry).fill_(False)
        bits = self.buf.view(BITS[self.buf.dtype])
        return listing(outside & (bits != self.nan_bits), f'{what}: guard written')


def guarded_like(x, dtype, stride=None, offset=0):
    """`x` (2-D, or 1-D as one row) copied into a Guarded view of `dtype`."""
    x2 = x if x.dim() == 2 else x.reshape(1, -1)
    g = Guarded(x2.shape[0], x2.shape[1], dtype, x.device, stride, offset)
    g.view.copy_(x2)
    return g


# ---- 1. column sums and the GELU backward ------------------------------------------------------------------------------------
# bias_gelu_bwd_kernel<ET, GELU, U>: grid (column chunks of 512, slices); wave w of slice y starts at row 4 y + w and walks
# with step = 4 * slices, U rows per trip of the main loop, one per trip of the tail.

COLSUM_U = {'gelu': 4, 'colsum': 8}
#  (rows, cols): {U: (fewest, most main-loop trips of a wave, fewest, most tail trips)} -- asserted against unrolled_trips
COLSUM_CASES = {
    (1, 8): {4: (0, 0, 0, 1), 8: (0, 0, 0, 1)},
    (3, 8): {4: (0, 0, 0, 1), 8: (0, 0, 0, 1)},
    (5, 520): {4: (0, 0, 0, 1), 8: (0, 0, 0, 1)},             # second column chunk: one active lane
    (16389, 8): {4: (1, 1, 0, 1), 8: (0, 0, 4, 5)},           # U = 4 main loop at 1024 slices
    (32773, 8): {4: (2, 2, 0, 1), 8: (1, 1, 0, 1)},           # U = 8 main loop at 1024 slices
    (8199, 520): {4: (1, 1, 0, 1), 8: (0, 0, 4, 5)},          # two column chunks
    (691, 12288): {4: (1, 1, 0, 1), 8: (0, 0, 4, 5)},
    (603, 12288): {4: (0, 1, 0, 3), 8: (0, 0, 3, 4)},         # some waves take a U = 4 trip, the others only the tail
    (1549, 12288): {4: (2, 2, 1, 2), 8: (1, 1, 1, 2)},        # U = 8: one trip plus a tail; U = 4: two trips plus a tail
}
COLSUM_MAIN_AND_TAIL = {4: [(16389, 8), (8199, 520), (691, 12288), (603, 12288), (1549, 12288)],
                        8: [(32773, 8), (1549, 12288)]}       # a wave with a main-loop trip AND a wave with a tail trip
BIAS_GELU_MAX_SLICES = 1024


def bias_gelu_slices(rows, cols):
    """bias_gelu_bwd_slices of csrc/bias_gelu.hip; the GPU test takes the number from bp_bias_grad_ws_floats instead."""
    chunks = (cols + 511) // 512
    return max(1, min((1024 + chunks - 1) // chunks, BIAS_GELU_MAX_SLICES, (rows + 3) // 4))


def unrolled_trips(rows, slices, u):
    """(main-loop trips, tail trips) of every wave of a column chunk: int64 tensors over the start rows 0 ... 4 * slices - 1."""
    step = 4 * slices
    r0 = torch.arange(step)
    main = (torch.div(rows - 1 - r0 - (u - 1) * step, u * step, rounding_mode='floor') + 1).clamp(min=0)
    tail = (torch.div(rows - 1 - (r0 + main * u * step), step, rounding_mode='floor') + 1).clamp(min=0)
    assert int((main * u + tail).sum()) == rows
    return main, tail


def trip_summary(rows, slices, u):
    main, tail = unrolled_trips(rows, slices, u)
    return int(main.min()), int(main.max()), int(tail.min()), int(tail.max())


def colsum_problem(rows, cols, device):
    """g: non-zero integers of magnitude <= 8 (even where pre = 0), pre in {+16, 0, -16}; fp64 expectations."""
    h = rc_hash(rows, cols, device, 1)
    sign = 1 - 2 * ((h >> 3) & 1)
    sel = (h >> 4) % 3
    g = torch.where(sel == 1, 2 * ((h & 3) + 1), (h & 7) + 1) * sign
    pre = (1 - sel) * 16
    slope = torch.tensor([1.0, 0.5, 0.0], dtype=torch.float64, device=device)[sel]   # gelu_tanh' at +16, 0, -16 as the kernel forms it
    g = g.double()
    return {'g': g, 'pre': pre.double(), 'dpre': g * slope, 'dbias': (g * slope).sum(0), 'colsum': g.sum(0)}


def gelu_r32(x):
    """r = 1 / (1 + exp2(2 u log2 e)) of csrc/bias_gelu.hip in fp32 torch (x fp32)."""
    u2 = (x * (0.044715 * (x * x) + 1.0)) * torch.tensor(2.0 * 0.7978845608028654 * LOG2E, dtype=torch.float32)
    return 1.0 / (1.0 + torch.exp2(u2))


def gelu_grad32(x):
    r = gelu_r32(x)
    du2 = torch.tensor(6.0 * 0.7978845608028654 * 0.044715, dtype=torch.float32) * (x * x) + 2.0 * 0.7978845608028654
    return (1.0 - r) * ((x * r) * du2 + 1.0)


def gelu_fwd32(x):
    return x * (1.0 - gelu_r32(x))


def exact_failures(got, want64, dtype, what):
    """torch.equal against the fp64 value rounded once; NaN (an element the call left unwritten) counts as wrong."""
    want = round_once(want64, dtype).to(got.device)
    return listing(~(got == want), what)


# ---- 2. bias + GELU forward --------------------------------------------------------------------------------------------------

GELU_FWD_MAX_WG = 8192        # csrc/bias_gelu.hip launch_bias_gelu_fwd: more workgroups than this -> grid-stride trips
GELU_FWD_CASES = [(3, 8), (257, 1032), (4100, 4096)]
GELU_FWD_VARIANTS = ['nobias', 'bias', 'bias_pre', 'bias_pre_inplace', 'nobias_inplace']


def gelu_fwd_trips(rows, cols):
    """(fewest, most) trips of a thread of bias_gelu_fwd_kernel."""
    nchunks = rows * (cols // 8)
    threads = 256 * min(-(-nchunks // 256), GELU_FWD_MAX_WG)
    return nchunks // threads, -(-nchunks // threads)


def gelu_fwd_problem(rows, cols, device, with_bias):
    """x + bias is an integer in [8, 120] or [-120, -8]: y == x + bias on the positive side (1 - r rounds to 1), +-0 on the
    negative one (r == 1), pre == x + bias."""
    h = rc_hash(rows, cols, device, 2)
    code = (h % 113 + 8) * (1 - 2 * ((h >> 9) & 1))
    bias = (_hash(torch.arange(cols, device=device) + 31) % 17 - 8) if with_bias else torch.zeros(cols, dtype=torch.long, device=device)
    return {'x': (code - bias).double(), 'bias': bias.double() if with_bias else None, 'pre': code.double(),
            'y': code.clamp(min=0).double()}


# ---- 3. cross-entropy --------------------------------------------------------------------------------------------------------

XENT_FILL = -128.0
XENT_LSE_TOL = 2.0 ** -20
XENT_SMALL = [1, 7, 8, 9, 2047, 2056, 4099]
XENT_BIG = [50257, 50264]
XENT_BIG_ROWS = 6 * 8 + 2 * 24 + 64
XENT_DTYPES = [torch.bfloat16, torch.float16, torch.float32]
XENT_SMOOTH = {'rows': 64, 'cols': 4099, 's': 0.1}


def odd_above(cols):
    return cols + 1 if cols % 2 == 0 else cols + 2


def xent_split(addr, cols, dtype):
    """(nhead, tail0) of the rows at byte addresses `addr` (int64 tensor): columns [0, nhead) and [tail0, cols) are walked
    element-wise, [nhead, tail0) in 16-byte loads (csrc/xentropy.hip)."""
    eb = 4 if dtype == torch.float32 else 2
    n = 16 // eb
    nhead = (((16 - (addr & 15)) & 15) // eb).clamp(max=cols)
    return nhead, nhead + (cols - nhead) // n * n


def row_addresses(view):
    return view.data_ptr() + torch.arange(view.shape[0]) * view.stride(0) * view.element_size()


def xent_small_needles(cols):
    return torch.arange(cols)


def xent_big_needles(cols, nhead, tail0):
    """Needle column of each of XENT_BIG_ROWS rows: first / last column, both ends of the head and of the tail (eight rows
    each: with an odd row stride that is one row per 16-byte phase), columns 256 * 8 * k +- 1, and 64 drawn columns."""
    r = torch.arange(XENT_BIG_ROWS)
    kinds = torch.stack([torch.zeros_like(nhead), torch.full_like(nhead, cols - 1), (nhead - 1).clamp(min=0),
                         nhead.clamp(max=cols - 1), (tail0 - 1).clamp(min=0), tail0.clamp(max=cols - 1)])
    j = _hash(r + 5) % cols
    j[:48] = kinds[r[:48] // 8, r[:48]]
    k = (r[48:96] - 48) // 2 + 1
    j[48:96] = 2048 * k + 2 * ((r[48:96] - 48) % 2) - 1
    return j


def xent_labels(j, cols):
    """Per row: the needle, another column, -100, cols (out of range), by row % 4."""
    r = torch.arange(j.numel())
    other = (j + 1 + _hash(r + 77) % max(cols - 1, 1)) % cols
    y = torch.where(r % 4 == 0, j, other)
    y = torch.where(r % 4 == 2, torch.full_like(j, -100), y)
    return torch.where(r % 4 == 3, torch.full_like(j, cols), y)


def xent_grads(rows):
    return torch.exp2(((torch.arange(rows) % 5) - 2).float())      # 1/4 ... 4


def xent_fill(view, j):
    """The needle rows, written into a (rows, cols) view of any stride."""
    view.fill_(XENT_FILL)
    view[torch.arange(view.shape[0], device=view.device), j.to(view.device)] = 0.0


def xent_want_loss(j, y, cols):
    """(value, exact): 0 exactly for a label out of range, else 0 or 128 within XENT_LSE_TOL."""
    inside = (y >= 0) & (y < cols)
    return torch.where(inside & (y != j), 128.0, 0.0).double(), ~inside


def xent_want_dx(j, y, g, cols):
    dx = torch.zeros(j.numel(), cols, dtype=torch.float64)
    r = torch.arange(j.numel())
    dx[r, j] = g.double()
    inside = (y >= 0) & (y < cols)
    dx[r[inside], y[inside]] -= g.double()[inside]
    return dx


def xent_fwd_failures(losses, lse, j, y, cols, what):
    losses, lse = losses.double().cpu(), lse.double().cpu()
    want, exact = xent_want_loss(j, y, cols)
    return (listing(~(lse.abs() <= XENT_LSE_TOL), f'{what}: lse')
            + listing(~((losses - want).abs() <= XENT_LSE_TOL), f'{what}: loss')
            + listing(exact & ~(losses == 0), f'{what}: loss of a label out of range'))


def smooth_problem():
    """Logits k / 8 with k in [-64, 64] (exact in every dtype), labels in range but for two rows."""
    c = XENT_SMOOTH
    h = rc_hash(c['rows'], c['cols'], 'cpu', 3)
    x = ((h % 129) - 64).double() / 8
    y = _hash(torch.arange(c['rows']) + 11) % c['cols']
    y[5], y[6] = -100, c['cols']
    return x, y, xent_grads(c['rows'])


def smooth_eval(x, y, g, s, dtype):
    """The kernel's formulas (csrc/xentropy.hip) in `dtype`: lse, loss, dx."""
    x = x.to(dtype)
    n = x.shape[1]
    s_t = torch.tensor(s, dtype=torch.float32).to(dtype)          # the kernel is handed an fp32 smoothing
    m = x.max(1).values
    lse = m + torch.log2(torch.exp2(x * LOG2E - (m * LOG2E)[:, None]).sum(1)) * LN2
    inside = (y >= 0) & (y < n)
    xy = x[torch.arange(x.shape[0]), y.clamp(0, n - 1)]
    loss = s_t * (lse - x.sum(1) / n) + torch.where(inside, (1 - s_t) * (lse - xy), torch.zeros_like(lse))
    hit = torch.zeros_like(x)
    hit[torch.arange(x.shape[0])[inside], y[inside]] = 1
    dx = g.to(dtype)[:, None] * (torch.exp2(x * LOG2E - (lse * LOG2E)[:, None]) - s_t / n - (1 - s_t) * hit)
    return lse, loss, dx


def smooth_bounds():
    """fp64 values and, per quantity, 4x the largest error of the fp32 evaluation of the same formulas."""
    x, y, g = smooth_problem()
    ref = smooth_eval(x, y, g, XENT_SMOOTH['s'], torch.float64)
    f32 = smooth_eval(x, y, g, XENT_SMOOTH['s'], torch.float32)
    return ref, [4 * float((a.double() - b).abs().max()) for a, b in zip(f32, ref)]


# ---- 4. add + LayerNorm forward ----------------------------------------------------------------------------------------------

LN_C, LN_A = 3.0, 64.0
LN_FWD_CH = {4: 1, 252: 1, 256: 1, 260: 2, 1028: 6, 1280: 6, 1536: 6, 1540: 8, 3076: 16, 4096: 16, 4100: 24, 6144: 24,
             6148: 32, 8192: 32}
LN_FWD_FEW_ROWS = {260: 1, 1280: 3, 4100: 5}
LN_CH_LIST = (1, 2, 3, 4, 6, 8, 12, 16, 24, 32)
#  name: (x0 is fp32, residual dtype: None = no residual in, 'f32' or '16', x_out, weights fp32)
LN_FWD_MODES = {'x16_w32': (False, None, True, True), 'x16_res32_w16': (False, 'f32', True, False),
                'x16_res16_w32': (False, '16', True, True), 'x32_w32': (True, None, True, True),
                'x32_res32_w32': (True, 'f32', False, True)}
# 4x the worst error of ln_fwd_eval in fp32 against the fp64 closed form over all cases, in units of the scale that
# ln_fwd_closed_form returns (measured by the host test: 1.12e-6, at cols = 6144, where the lane that holds the spike adds up
# to 95 squares of 1.1e-4 to a sum of 4095, each below half an ulp: evaluated with torch.sum the same formulas are 2.3e-7 off)
LN_FWD_F32_BOUND = 4.5e-6
LN_FWD_MUTANT_FACTOR = 100


def ln_ch(cols, listed=LN_CH_LIST):
    chunks = -(-cols // 256)
    return next(c for c in listed if c >= chunks)


def ln_spike_columns(cols, rows=None):
    """Spike column of each row: every column up to 1540 wide; beyond that the first and last columns of the first and last
    lane of every 256-column chunk, the last lane of the row, and 64 drawn columns.  `rows`: that many drawn columns."""
    if rows is not None:
        return _hash(torch.arange(rows) + cols) % cols
    if cols <= 1540:
        return torch.arange(cols)
    base = torch.arange(0, cols, 256)[:, None] + torch.tensor([0, 3, 4, 252, 255])[None, :]
    js = torch.cat([base.flatten(), torch.tensor([cols - 4, cols - 1]), _hash(torch.arange(64) + cols) % cols])
    return js[js < cols]


def ln_weights(cols):
    h = _hash(torch.arange(cols) + 911)
    gamma = ((h & 3) + 1) * (1 - 2 * ((h >> 2) & 1))
    beta = torch.where((h >> 5) % 2 == 0, torch.zeros_like(h), (h >> 6) % 5 - 2)
    return gamma.double(), beta.double()


def ln_fwd_problem(cols, js, residual):
    """x0 = 3 with a spike of 64 at column js[i]; the residual (+2, and the spike moved to another column) or None.  All fp64
    holding integers; `spike`: where the spike of the SUM sits, `c`: its constant."""
    rows = js.numel()
    r = torch.arange(rows)
    x0 = torch.full((rows, cols), LN_C, dtype=torch.float64)
    x0[r, js] += LN_A
    x1, spike, c = None, js, LN_C
    if residual:
        spike = (js + 1 + cols // 2) % cols
        x1 = torch.full((rows, cols), 2.0, dtype=torch.float64)
        x1[r, js] -= LN_A
        x1[r, spike] += LN_A
        c = LN_C + 2.0
    gamma, beta = ln_weights(cols)
    return {'x0': x0, 'x1': x1, 'x': x0 if x1 is None else x0 + x1, 'spike': spike, 'c': c, 'gamma': gamma, 'beta': beta}


def eps64():
    return torch.tensor(EPS, dtype=torch.float32).double()


def ln_fwd_closed_form(prob):
    """z (fp64) and the tolerance scale |gamma| (|x| + |mu|) rs + |beta| of every element."""
    rows, n = prob['x'].shape
    mu = prob['c'] + LN_A / n
    rs = 1.0 / torch.sqrt(LN_A ** 2 * (n - 1) / n ** 2 + eps64())
    d = torch.full((rows, n), prob['c'] - mu, dtype=torch.float64)
    d[torch.arange(rows), prob['spike']] += LN_A
    z = d * rs * prob['gamma'] + prob['beta']
    return z, prob['gamma'].abs() * (prob['x'].abs() + mu) * rs + prob['beta'].abs()


def wave_row_sum(v, ch):
    """Row sums of v (rows, cols) in the order of add_layer_norm_kernel<CH>: lane l of the row's wave owns columns
    (c * 64 + l) * 4 + i and adds them one after the other, c = 0 ... CH - 1, i = 0 ... 3; the 64 lanes then meet in an xor
    butterfly (32, 16, ... 1).  In fp32 a lane that has taken the spike's square absorbs the small squares that follow it:
    that is the kernel's own rounding, and the reason the bound is measured on this order and not on torch.sum."""
    rows, cols = v.shape
    pad = v.new_zeros(rows, ch * 256)
    pad[:, :cols] = v
    pad = pad.view(rows, ch, 64, 4)
    lane = v.new_zeros(rows, 64)
    for c in range(ch):
        for i in range(4):
            lane = lane + pad[:, c, :, i]
    idx = torch.arange(64)
    for m in (32, 16, 8, 4, 2, 1):
        lane = lane + lane[:, idx ^ m]
    return lane[:, 0]


def ln_fwd_eval(prob, dtype=torch.float32, mean_weight=1.0, var_weight=1.0):
    """The kernel's operation order in `dtype`: two sums over n (wave_row_sum), one reciprocal square root, the affine step.
    The spike enters the mean with `mean_weight` and the variance with `var_weight` (mutants: 0 = left out, 2 = twice)."""
    x = prob['x'].to(dtype)
    n = x.shape[1]
    ch = ln_ch(n)
    r = torch.arange(x.shape[0])
    at = (r, prob['spike'])
    inv_n = torch.tensor(1.0, dtype=dtype) / n
    w = torch.ones_like(x)
    w[at] = mean_weight
    mu = wave_row_sum(x * w, ch) * inv_n
    d = x - mu[:, None]
    w[at] = var_weight
    m2 = wave_row_sum(d * d * w, ch)
    rs = torch.rsqrt(m2 * inv_n + torch.tensor(EPS, dtype=torch.float32).to(dtype))
    return d * rs[:, None] * prob['gamma'].to(dtype) + prob['beta'].to(dtype)


def ln_fwd_failures(z, prob, out_dtype, what):
    """fp32 z: within LN_FWD_F32_BOUND scales of the closed form; 16-bit z: within one ulp of the rounded closed form."""
    want, scale = ln_fwd_closed_form(prob)
    z = z.double().cpu()
    if out_dtype == torch.float32:
        return listing(~((z - want).abs() <= LN_FWD_F32_BOUND * scale), f'{what}: z')
    rounded = want.float().to(out_dtype).double()
    return listing(~((z - rounded).abs() <= ulp(rounded, out_dtype)), f'{what}: z')


# ---- 5. add + LayerNorm backward ---------------------------------------------------------------------------------------------

LN_BWD_COLS = [4, 256, 260, 1028, 1280, 1536, 1540, 2048]
LN_BWD_ROWS = [1, 2, 5, 4096, 4097, 4100, 8195, 12291]
LN_BWD_CH_LIST = (1, 2, 3, 4, 6, 8)
LN_BWD_TRIPS = {1: (0, 1), 2: (0, 1), 5: (0, 1), 4096: (1, 1), 4097: (1, 2), 4100: (1, 2), 8195: (2, 3), 12291: (3, 4)}
# 4x the worst error of the fp32 evaluation (ln_bwd_rows / ln_bwd_fold in fp32) against fp64, in units of each quantity's scale
# (measured by the host test: dx 7.75e-7 at 12291 x 260, dgamma 2.54e-7 at 2 x 2048, dcolscale 2.03e-7 at 2 x 1280)
LN_BWD_BOUND = {'dx': 3.15e-6, 'dgamma': 1.03e-6, 'dcolscale': 8.2e-7}


def ln_bwd_cases():
    """(cols, rows, dx_in, dx1, colscale): every shape of the issue; the three options rotate so that each is on and off at
    rows of a second and third trip."""
    cases = []
    for ci, cols in enumerate(LN_BWD_COLS):
        for ri, rows in enumerate(LN_BWD_ROWS):
            if rows > 4100 and cols > 1280:
                continue
            k = ci + ri
            cases.append((cols, rows, k % 2 == 0, (k // 2) % 2 == 0, (k // 4) % 2 == 0))
    return cases


def ln_bwd_nwg(rows, cap):
    return min((rows + 3) // 4, cap)


def ln_bwd_trips(rows, cap):
    """(fewest, most) rows a wave of add_layer_norm_bwd_kernel takes."""
    per = 4 * ln_bwd_nwg(rows, cap)
    return rows // per, -(-rows // per)


def ln_bwd_problem(rows, cols, device, colscale):
    """dz: integers of magnitude <= 8, zero on the rows with row % 5 == 2; x, dx_in, x0: integers in [-8, 8]; gamma: k / 4;
    colscale: 1/2, 1 or 2.  fp64, on `device`."""
    h = rc_hash(rows, cols, device, 4)
    live = (torch.arange(rows, device=device) % 5 != 2)[:, None]
    dz = ((h & 7) + 1) * (1 - 2 * ((h >> 3) & 1)) * live
    x = (h >> 8) % 17 - 8
    dx_in = (h >> 14) % 17 - 8
    x0 = (h >> 20) % 17 - 8
    hc = _hash(torch.arange(cols, device=device) + 313)
    gamma = ((hc % 15) + 1).double() * (1 - 2 * ((hc >> 7) & 1)) / 4
    cs = torch.exp2(((hc >> 9) % 3 - 1).double()) if colscale else None
    return {'dz': dz.double(), 'x': x.double(), 'dx_in': dx_in.double(), 'x0': x0.double(), 'gamma': gamma, 'cs': cs,
            'live': live[:, 0]}


def ln_bwd_rows(prob, dtype, dx_in):
    """The row-wise formulas in `dtype`: dx (before the colscale), its tolerance scale, the terms of dgamma and theirs."""
    dz, x, gamma = (prob[k].to(dtype) for k in ('dz', 'x', 'gamma'))
    n = x.shape[1]
    inv_n = torch.tensor(1.0, dtype=dtype, device=x.device) / n
    mu = x.sum(1, keepdim=True) * inv_n
    d = x - mu
    rs = torch.rsqrt((d * d).sum(1, keepdim=True) * inv_n + torch.tensor(EPS, dtype=torch.float32).to(dtype))
    xhat = d * rs
    dy = dz * gamma
    c2 = dy.sum(1, keepdim=True) * inv_n
    c1 = (dy * xhat).sum(1, keepdim=True) * inv_n
    dx = rs * (dy - c2 - xhat * c1)
    xabs = (x.abs() + mu.abs()) * rs                       # what bounds the rounding of xhat = (x - mu) rs, not |xhat| itself
    scale = rs * (dy.abs() + c2.abs() + xabs * c1.abs())
    if dx_in:
        dx = dx + prob['dx_in'].to(dtype)
        scale = scale + prob['dx_in'].to(dtype).abs()
    return dx, scale, dz * xhat, dz.abs() * xabs


def ln_bwd_fold(terms, n_wg, trip_weight=None):
    """Column sums of `terms` (rows, cols) in the kernel's order, in the terms' dtype: a wave adds its rows trip after trip,
    the four waves of a workgroup fold in order, ln_bwd_reduce_kernel adds the partial rows r % 16 == s in order and then
    the 16 slices.  trip_weight: {trip: weight} for the mutants (0: a trip dropped, 2: counted twice)."""
    rows, cols = terms.shape
    per = 4 * n_wg
    trips = -(-rows // per)
    pad = terms.new_zeros(trips * per, cols)
    pad[:rows] = terms
    pad = pad.view(trips, n_wg, 4, cols)
    acc = terms.new_zeros(n_wg, 4, cols)
    for t in range(trips):
        acc += pad[t] * (trip_weight or {}).get(t, 1)
    part = acc[:, 0]
    for w in range(1, 4):
        part = part + acc[:, w]
    groups = -(-n_wg // 16)
    pad = terms.new_zeros(groups * 16, cols)
    pad[:n_wg] = part
    pad = pad.view(groups, 16, cols)
    sl = terms.new_zeros(16, cols)
    for i in range(groups):
        sl += pad[i]
    out = sl[0]
    for s in range(1, 16):
        out = out + sl[s]
    return out


def ln_bwd_eval(prob, dtype, n_wg, dx_in, trip_weight=None):
    """dict of dx0, dx1, dgamma, dbeta, dcolscale and the tolerance scales, evaluated in `dtype`."""
    dx, scale, dg_terms, dg_scale = ln_bwd_rows(prob, dtype, dx_in)
    out = {'dx1': dx, 'dx_scale': scale, 'dx0': dx, 'dx0_scale': scale,
           'dgamma': ln_bwd_fold(dg_terms, n_wg, trip_weight), 'dgamma_scale': dg_scale.sum(0),
           'dbeta': ln_bwd_fold(prob['dz'].to(dtype), n_wg, trip_weight)}
    if prob['cs'] is not None:
        dcs_terms = dx * prob['x0'].to(dtype)
        out.update(dx0=dx * prob['cs'].to(dtype), dx0_scale=scale * prob['cs'].to(dtype),
                   dcolscale=ln_bwd_fold(dcs_terms, n_wg, trip_weight), dcolscale_scale=(scale * prob['x0'].to(dtype).abs()).sum(0))
    return out


def ln_bwd_exact_failures(got, prob, dx_in, w_dtype, what):
    """The criteria that hold in every mode: dbeta == sum of dz (rounded once to the weights' dtype); on rows with dz = 0,
    dx1 == dx_in and dx0 == dx_in * colscale bit for bit (0 without a dx_in)."""
    bad = exact_failures(got['dbeta'], prob['dz'].sum(0), w_dtype, f'{what}: dbeta')
    dead = ~prob['live']
    passed = prob['dx_in'][dead] if dx_in else torch.zeros_like(prob['dx_in'][dead])
    if got.get('dx1') is not None:
        bad += listing(~(got['dx1'][dead].double() == passed), f'{what}: dx1 on rows with dz = 0')
    scaled = passed if prob['cs'] is None else passed * prob['cs']
    bad += listing(~(got['dx0'][dead].double() == scaled), f'{what}: dx0 on rows with dz = 0')
    return bad


def ln_bwd_bound_failures(got, ref, what):
    """All-fp32 mode: dx0, dx1, dgamma, dcolscale against the fp64 evaluation `ref` within LN_BWD_BOUND scales."""
    bad = []
    for name, key in (('dx0', 'dx'), ('dx1', 'dx'), ('dgamma', 'dgamma'), ('dcolscale', 'dcolscale')):
        if got.get(name) is None or name not in ref:
            continue
        scale = ref['dx0_scale' if name == 'dx0' else 'dx_scale' if name == 'dx1' else name + '_scale']
        bad += listing(~((got[name].double() - ref[name]).abs() <= LN_BWD_BOUND[key] * scale), f'{what}: {name}')
    return bad


def ln_bwd_ratios(got, ref):
    """Largest |got - ref| / scale per quantity (dx: over dx0 and dx1)."""
    out = {}
    for name, key in (('dx0', 'dx'), ('dx1', 'dx'), ('dgamma', 'dgamma'), ('dcolscale', 'dcolscale')):
        if got.get(name) is None or name not in ref:
            continue
        scale = ref['dx0_scale' if name == 'dx0' else 'dx_scale' if name == 'dx1' else name + '_scale']
        err = (got[name].double() - ref[name]).abs()
        ratio = torch.where(scale > 0, err / scale.clamp(min=1e-300), torch.where(err > 0, torch.full_like(err, float('inf')), err))
        out[key] = max(out.get(key, 0.0), float(ratio.max()))
    return out


# ---- 6. causal softmax backward ----------------------------------------------------------------------------------------------

SOFTMAX_CASES = {8: 1, 504: 1, 512: 1, 520: 2, 1032: 4, 2056: 8, 4096: 8}     # S: CH
SOFTMAX_REFUSED = [4104, 12]
SOFTMAX_SCALE = 0.5
SOFTMAX_POISON = 777.0


def softmax_ch(s):
    return next(c for c in (1, 2, 4, 8) if c >= -(-s // 512))


def softmax_matrices(s):
    return 3 if s <= 1032 else 1


def softmax_problem(s, n, device):
    """alpha[t, :] = 2^-m on its first 2^m columns, m = floor(log2(t + 1)); dA integers of magnitude <= 8 on and below the
    diagonal, 777 above it.  The fp64 result is exact in fp32."""
    t = torch.arange(s, device=device)
    m = ((t + 1)[:, None] >= (1 << torch.arange(13, device=device))[None, :]).sum(1) - 1
    col = torch.arange(s, device=device)[None, :]
    alpha = torch.where(col < (1 << m)[:, None], torch.exp2(-m.double())[:, None], torch.zeros((), dtype=torch.float64, device=device))
    h = _hash((torch.arange(n, device=device)[:, None, None] * s + t[None, :, None]) * 4099 + col[None])
    da = (((h & 7) + 1) * (1 - 2 * ((h >> 3) & 1))).double()
    below = (col <= t[:, None])[None]
    da = torch.where(below, da, torch.full_like(da, SOFTMAX_POISON))
    alpha = alpha[None].expand(n, s, s)
    acc = (alpha * torch.where(below, da, torch.zeros_like(da))).sum(-1, keepdim=True)
    want = torch.where(below, SOFTMAX_SCALE * alpha * (da - acc), torch.zeros_like(da))
    return {'alpha': alpha.contiguous(), 'da': da, 'want': want, 'acc': acc}
