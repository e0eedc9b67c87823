"""GPU: bp_sense_attribute (csrc/sense_attribute.hip) and src/utils/sense_attribution.py on the HIP path.

  needles      +-1 position codes as keys and queries (tests/decode_needles.py) at a scale that puts every other key 128
               below the needle: its e is exactly 1, every other e is exactly 0, so p is 1 / 0; table rows and vectors are
               small integers, every dot exact in fp32 in any order -> the whole output is compared as int32 bits.  Rows and
               keys behind the query, and everything the index does not name, are NaN: reading one of them shows.
  drawn        against the float64 restatement (tests/sense_attribution_ref.py); the bound is 4 x the error of an fp32 torch
               evaluation on the CPU of the test's own inputs, in units of p_j sum_c |row_c| |vec_c|, plus one fp32 ulp
  model        the (k, S) sum against the fp32 twin's logit (whole-model rule, 3 x the 16-bit eager twin's error), the weights
               against the twin's alpha row (kernel rule, 2 x)
  determinism  repeated calls, capture and three replays with query_pos rewritten on the device
  layer        sense_contributions / contextual_localize / top_contributions against the CPU twin fed the same qk / table
Every output and the workspace lie inside NaN buffers whose guards and stride gaps must keep their bits."""
import numpy as np
import pytest
import torch

import decode_needles as N
import sense_attribution_ref as R
from decode_support import DEV, _bp, _fp32_twin, _model, _within_2x

pytestmark = pytest.mark.gpu

DTYPES = {'bf16': torch.bfloat16, 'fp16': torch.float16}
NAN = float('nan')
NAN_BITS = torch.full((1,), NAN).view(torch.int32).item()


class Guarded:
    """A strided fp32 view inside a flat NaN buffer with a guard on either side."""

    def __init__(self, shape, strides, guard=64):
        span = 1 + sum((n - 1) * s for n, s in zip(shape, strides))
        self.buf = torch.full((guard + span + guard,), NAN, device=DEV)
        self.geometry = (tuple(shape), tuple(strides), guard)
        self.view = self.buf.as_strided(*self.geometry)

    def guard_intact(self):
        outside = torch.ones(self.buf.numel(), dtype=torch.bool, device=DEV)
        outside.as_strided(*self.geometry).fill_(False)
        return bool((self.buf.view(torch.int32)[outside] == NAN_BITS).all())


def _gapped(nq, nvec, k, s, gaps):
    """Element strides (query, vector, sense, 1) with `gaps` = extra elements behind a row, a sense block, a vector block."""
    o_ss = s + gaps[0]
    o_vs = k * o_ss + gaps[1]
    return (nvec * o_vs + gaps[2], o_vs, o_ss, 1)


def _launch(qk, table, index, qs, qp, vec, scale, gaps=(0, 0, 0), want_probs=True):
    """One call through the C ABI with guarded out / probs / ws: (out view, probs view or None)."""
    bp = _bp()
    b, s, _, k, dk = qk.shape
    nq, nvec, dout = vec.shape
    out = Guarded((nq, nvec, k, s), _gapped(nq, nvec, k, s, gaps))
    pst = _gapped(nq, 1, k, s, gaps)
    probs = Guarded((nq, k, s), (pst[0], pst[2], 1)) if want_probs else None
    ws_floats = bp.lib().bp_sense_attribute_ws_floats(nq, k)
    assert ws_floats == 2 * nq * k
    ws = Guarded((ws_floats,), (1,))
    bp._call('bp_sense_attribute', DEV, qk.data_ptr(), table.data_ptr(), index.data_ptr(), qs.data_ptr(), qp.data_ptr(),
             vec.data_ptr(), out.view.data_ptr(), probs.view.data_ptr() if want_probs else None, ws.view.data_ptr(), ws_floats,
             b, s, k, dk, dout, nq, nvec, table.shape[0], qk.stride(0), qk.stride(1), qk.stride(2), qk.stride(3),
             table.stride(0), table.stride(1), index.stride(0), vec.stride(0), vec.stride(1),
             *out.view.stride()[:3], *(probs.view.stride()[:2] if want_probs else (0, 0)), float(scale),
             1 if qk.dtype == torch.bfloat16 else 0)
    torch.cuda.synchronize()
    assert out.guard_intact(), 'out: a guard or a stride gap was written'
    assert ws.guard_intact() and torch.isfinite(ws.view).all(), 'ws: written outside the (m, Z) pairs, or a pair left unwritten'
    if want_probs:
        assert probs.guard_intact(), 'probs: a guard or a stride gap was written'
    return out.view, (probs.view if want_probs else None)


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---- needles ----------------------------------------------------------------------------------------------------------------------------------
# (seqlen, d_k, d_out, senses, vectors): every seqlen, d_k, d_out (NCH = 1 .. 4, whole and partial last chunks), sense and
# vector count of the list, each d_k wide enough for distinct codes of its positions
NEEDLE_CASES = [(1, 8, 8, 1, 1), (2, 16, 384, 4, 4), (4, 48, 512, 16, 1), (5, 160, 520, 4, 4), (63, 640, 768, 1, 1),
                (64, 8, 1032, 64, 4), (65, 48, 2048, 16, 4), (257, 16, 768, 16, 1), (257, 48, 8, 64, 4)]


def _needle_positions(i):
    """Needles for a query at i: 0, i itself, and either side of a 4-position block border inside the prefix."""
    border = (i // 2) // 4 * 4
    return sorted({j for j in (0, i, border - 1, border) if 0 <= j <= i})


@pytest.mark.parametrize('dtype', sorted(DTYPES))
@pytest.mark.parametrize('case', NEEDLE_CASES, ids=lambda c: 'S%d-dk%d-d%d-k%d-v%d' % c)
def test_needles_bit_for_bit(case, dtype):
    s, dk, dout, k, nvec = case
    dt = DTYPES[dtype]
    assert s - 1 <= N.max_length(dk)
    # one query position per sample: 0, the last and the first position of a workgroup's four, the last of the row
    qpos = sorted({i for i in (0, 3, 4, s - 1) if i < s})
    batch = len(qpos)
    ar_s, ar_k = torch.arange(s, device=DEV), torch.arange(k, device=DEV)
    needle = torch.zeros((batch, k), dtype=torch.long, device=DEV)
    for b, i in enumerate(qpos):
        cand = _needle_positions(i)
        needle[b] = torch.tensor([cand[(l + b) % len(cand)] for l in range(k)], device=DEV)
    visible = ar_s[None, :] <= torch.tensor(qpos, device=DEV)[:, None]                          # (B, S)
    qk = torch.full((batch, s, 2, k, dk), NAN, device=DEV)
    qk[:, :, 1] = torch.where(visible[:, :, None, None], N.code(ar_s, dk)[None, :, None, :], NAN)   # keys behind i_b: NaN
    for b, i in enumerate(qpos):
        qk[b, i, 0] = N.code(needle[b], dk)                                                    # the only query row that is read
    qk = qk.to(dt)
    # row(b, j) = 2 (b S + j) in front of i_b and at it, an odd row behind it; the odd rows are NaN
    rows = 2 * batch * s
    slot = torch.arange(batch, device=DEV)[:, None] * s + ar_s[None, :]
    index = torch.where(visible, 2 * slot, 2 * slot + 1).int()
    table = torch.full((rows, k, dout), NAN, device=DEV)
    table[0::2] = N.values(torch.arange(rows // 2, device=DEV)[:, None] * 64 + ar_k[None, :], dout)
    table = table.to(dt)
    # queries: the samples in reverse order, the first one twice
    order = list(range(batch))[::-1] + [0]
    qs = torch.tensor(order, dtype=torch.int32, device=DEV)
    qp = torch.tensor([qpos[b] for b in order], dtype=torch.int32, device=DEV)
    nq = len(order)
    vec = (N.values(torch.arange(nq * nvec, device=DEV) + 7777, dout) * 0.5).round().view(nq, nvec, dout)   # integers in [-4, 4]
    vec[-1] = vec[batch - 1]                                                                   # the duplicate of sample 0's query
    scale = 64.0 / N.reps(dk)                                                                  # 128 between the needle and any other key
    out, probs = _launch(qk, table, index, qs, qp, vec, scale, gaps=(3, 5, 7))
    # expected: p is exactly 1 at the needle and 0 elsewhere; the dots are exact integers below 2^24
    content = torch.where(visible[:, :, None, None], table[index.long()].double(), 0.0)         # (B, S, k, d)
    dots = torch.einsum('nslc,nvc->nvls', content[qs.long()], vec.double()).float()             # (nq, nvec, k, S)
    assert dots.abs().max() < 2 ** 24
    p = (ar_s[None, None, :] == needle[qs.long()][:, :, None]).float()                          # (nq, k, S)
    want = p[:, None] * dots                                                                    # +-0 where p = 0, as the kernel's product
    want = torch.where(visible[qs.long()][:, None, None, :], want, 0.0)
    assert torch.equal(_bits(probs), _bits(p)), 'probs: exactly 1 at the needle, 0 elsewhere'
    bad = _bits(out) != _bits(want)
    assert not bad.any(), f'{int(bad.sum())} entries differ, first at {bad.nonzero()[:4].tolist()}'
    assert (want != 0).any(), 'the needles carry non-zero shares'
    assert torch.equal(_bits(out[-1]), _bits(out[batch - 1])), 'the duplicated query'
    again, _ = _launch(qk, table, index, qs, qp, vec, scale, gaps=(0, 0, 0), want_probs=False)
    assert torch.equal(_bits(again), _bits(out)), 'without probs, dense strides: the same bits'
    # every sample alone, the keys and the rows of all the others NaN as well: a query reads its own sample only
    for n, b in enumerate(order[:batch]):
        own = torch.arange(batch, device=DEV) == b
        qk1 = torch.where(own[:, None, None, None, None], qk, torch.full_like(qk, NAN))
        table1 = torch.where((own[:, None] & visible).repeat_interleave(2, dim=1).reshape(-1)[:, None, None], table,
                             torch.full_like(table, NAN))
        alone, alone_p = _launch(qk1, table1, index, qs[n:n + 1], qp[n:n + 1], vec[n:n + 1], scale)
        assert torch.equal(_bits(alone[0]), _bits(out[n])) and torch.equal(_bits(alone_p[0]), _bits(probs[n])), (n, b)


# ---- drawn parity ------------------------------------------------------------------------------------------------------------------------------

def _ulp32(x):
    return np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)


@pytest.mark.parametrize('dtype', sorted(DTYPES))
@pytest.mark.parametrize('shape', [(3, 130, 16, 48, 768, 2), (2, 33, 4, 160, 640, 3)], ids=lambda c: 'B%d-S%d-k%d-dk%d-d%d-v%d' % c)
def test_drawn_parity_with_the_restatement(shape, dtype):
    from src.utils import sense_attribution as SA
    batch, s, k, dk, d, nvec = shape
    dt = DTYPES[dtype]
    g = torch.Generator(device=DEV).manual_seed(s + k)
    proj = torch.full((batch, s, 2 * d + 16), NAN, device=DEV).to(dt)                           # a (B, S, 2 d) projection inside wider rows
    proj[..., :2 * d] = (torch.randn(batch, s, 2 * d, device=DEV, generator=g) * 1.5).to(dt)
    qk = proj[..., :2 * d].view(batch, s, 2, k, dk)
    assert not qk.is_contiguous()
    rows = 211
    table = torch.randn(rows, k, d, device=DEV, generator=g).to(dt)
    index = torch.randint(0, rows, (batch, s), device=DEV, generator=g, dtype=torch.int32)
    index[0, 1], index[1, 2], index[-1, -1] = rows, 2 ** 31 - 1, -1                             # beyond the table: the last row
    last = s - 1
    # samples interleaved, a duplicate, out-of-range entries and their clamped twins
    pairs = [(0, last), (1, 64), (0, 3), (batch - 1, last), (1, 64), (0, 0), (1, 7),
             (-1, 3), (0, s), (batch, last), (batch - 1, -1), (batch - 1, 0)]
    twins = {7: 2, 8: 0, 9: 3, 10: 11}
    pairs = [(b, min(i, last) if i == 64 else i) for b, i in pairs]
    qs = torch.tensor([b for b, _ in pairs], dtype=torch.int32, device=DEV)
    qp = torch.tensor([i for _, i in pairs], dtype=torch.int32, device=DEV)
    vec = torch.randn(len(pairs), nvec, d, device=DEV, generator=g)
    vec[4] = vec[1]
    for wild, tame in twins.items():
        vec[wild] = vec[tame]
    scale = dk ** -0.5
    out, probs = _launch(qk, table, index, qs, qp, vec, scale, gaps=(2, 11, 5))
    for wild, tame in twins.items():
        assert torch.equal(_bits(out[wild]), _bits(out[tame])) and torch.equal(_bits(probs[wild]), _bits(probs[tame])), (wild, tame)
    assert torch.equal(_bits(out[4]), _bits(out[1])), 'the duplicated query'
    want, want_p, unit = R.sense_attribute(qk, table, index.cpu(), qs.cpu(), qp.cpu(), vec, scale)
    cpu, cpu_p = SA._eager_sense_attribute(qk.cpu(), table.cpu(), index.cpu(), qs.cpu(), qp.cpu(), vec.cpu(), scale, True)
    live = unit > 0
    cpu_fig = (np.abs(cpu.double().numpy() - want)[live] / unit[live]).max()
    cpu_fig_p = (np.abs(cpu_p.double().numpy() - want_p)[want_p > 0] / want_p[want_p > 0]).max()
    err = np.abs(out.double().cpu().numpy() - want)
    err_p = np.abs(probs.double().cpu().numpy() - want_p)
    gpu_fig = (err[live] / unit[live]).max()
    gpu_fig_p = (err_p[want_p > 0] / want_p[want_p > 0]).max()
    print(f'drawn {shape} {dtype}: error in units of p sum|row||vec|: fp32 torch on the CPU {cpu_fig:.3e}, kernel {gpu_fig:.3e}; '
          f'of p: CPU {cpu_fig_p:.3e}, kernel {gpu_fig_p:.3e}')
    assert (err <= 4 * cpu_fig * unit + _ulp32(unit)).all()
    assert (err_p <= 4 * cpu_fig_p * want_p + _ulp32(want_p)).all()
    behind = (np.arange(s)[None, :] > np.clip(qp.cpu().numpy(), 0, last)[:, None])
    assert (out.cpu().numpy()[np.broadcast_to(behind[:, None, None, :], out.shape)].view(np.int32) == 0).all()
    assert (probs.cpu().numpy()[np.broadcast_to(behind[:, None, :], probs.shape)].view(np.int32) == 0).all()


# ---- determinism, capture -----------------------------------------------------------------------------------------------------------------------

def test_repeated_calls_and_graph_replays_are_bit_identical():
    bp = _bp()
    batch, s, k, dk, d, nvec, nq = 2, 70, 16, 48, 768, 2, 5
    g = torch.Generator(device=DEV).manual_seed(11)
    qk = (torch.randn(batch, s, 2, k, dk, device=DEV, generator=g) * 1.5).bfloat16()
    table = torch.randn(97, k, d, device=DEV, generator=g).bfloat16()
    index = torch.randint(0, 97, (batch, s), device=DEV, generator=g, dtype=torch.int32)
    qs = torch.tensor([0, 1, 0, 1, 1], dtype=torch.int32, device=DEV)
    positions = [torch.tensor(p, dtype=torch.int32, device=DEV) for p in ([69, 3, 17, 0, 40], [0, 69, 4, 33, 8], [12, 12, 68, 1, 5])]
    vec = torch.randn(nq, nvec, d, device=DEV, generator=g)
    scale = dk ** -0.5
    eager = [bp.sense_attribute(qk, table, index, qs, p, vec, scale, want_probs=True) for p in positions]
    for p, (o, pr) in zip(positions, eager):
        o2, pr2 = bp.sense_attribute(qk, table, index, qs, p, vec, scale, want_probs=True)
        assert torch.equal(_bits(o), _bits(o2)) and torch.equal(_bits(pr), _bits(pr2)), 'repeated calls'
    qp = positions[0].clone()
    out = torch.empty((nq, nvec, k, s), device=DEV)
    probs = torch.empty((nq, k, s), device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        bp.sense_attribute(qk, table, index, qs, qp, vec, scale, out=out, probs=probs)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        bp.sense_attribute(qk, table, index, qs, qp, vec, scale, out=out, probs=probs)
    for p, (o, pr) in zip(positions, eager):
        qp.copy_(p)                                            # rewritten on the device: the host never read the queries
        out.fill_(NAN)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(_bits(out), _bits(o)) and torch.equal(_bits(probs), _bits(pr)), 'a replay equals the eager call'


# ---- model level -------------------------------------------------------------------------------------------------------------------------------

S_MODEL = 96


@pytest.fixture(scope='module', params=['small', 'mini_k4'])
def hip_model(request):
    _bp()
    model = _model(request.param)
    ids = torch.randint(0, 4096, (2, S_MODEL), device=DEV, generator=torch.Generator(device=DEV).manual_seed(3))
    return request.param, model, ids


def _eager16_twin(model):
    """The eager op sequence in the model's own 16-bit type with the same weights: the yardstick of DESIGN.md section 2."""
    from src.models.backpack import BackpackConfig, BackpackLMHeadModel
    kw = {k: v for k, v in model.config.to_dict().items() if k in ('n_embd', 'n_head', 'n_layer', 'num_content_vectors',
                                                                   'vocab_size', 'n_positions')}
    twin = BackpackLMHeadModel(BackpackConfig(scale_attn_by_inverse_layer_idx=True, use_flash_attn=False, **kw))
    twin.load_state_dict({k: v.float() for k, v in model.state_dict().items()})
    return twin.to(device=DEV, dtype=model.lm_head.weight.dtype).eval()


def test_the_shares_sum_to_the_fp32_twins_logit(hip_model):
    from src.utils import sense_attribution as SA
    name, model, ids = hip_model
    twin, eager = _fp32_twin(model), _eager16_twin(model)
    pairs = [(0, 37), (1, 37), (0, S_MODEL - 1), (1, S_MODEL - 1)]
    targets = torch.tensor([[5, 1234, 4000]] * len(pairs), device=DEV)
    res = SA.sense_contributions(model, ids, pairs, target_ids=targets, return_probs=True)
    assert res.contributions.is_cuda and res.contributions.shape == (4, 3, model.transformer.num_content_vectors, S_MODEL)
    with torch.no_grad():
        ref = twin(ids).logits.float()
        low = eager(ids).logits.float()
        alpha_ref = twin.transformer.contextualization_attn(twin.transformer.gpt2_model(ids)).float()
        alpha_low = eager.transformer.contextualization_attn(eager.transformer.gpt2_model(ids)).float()
    want = torch.stack([ref[b, i, targets[0]] for b, i in pairs])
    base = torch.stack([low[b, i, targets[0]] for b, i in pairs])
    # DESIGN.md section 2, whole models: 3 x the error of the 16-bit eager model, with the floor of decode_support._close_drawn
    # (two units of the MODEL's 16-bit rounding at the result's range; the sum itself is fp32)
    err = (res.logits - want).abs().max().item()
    yard = (base - want).abs().max().item()
    floor = 2.0 * 2.0 ** -8 * want.abs().max().item()
    print(f'{name}: sum of the shares against the fp32 twin {err:.3e}, 16-bit eager twin {yard:.3e}, floor {floor:.1e}')
    assert torch.isfinite(res.logits).all() and err <= 3.0 * yard + floor + 1e-5, (name, err, yard, floor)
    # DESIGN.md section 2, kernels: 2 x the error of the same-dtype eager path, applied as everywhere in this suite to the
    # whole output of the call (all four rows).  What separates either 16-bit path from the twin is the trunk in front of the
    # sharpened softmax, not the weights' own arithmetic (1e-6, see the drawn parity), so ONE row against ONE row is a draw:
    # measured per query on the MI355X (small): 7.9e-2 / 9.5e-2, 6.0e-2 / 9.5e-2, 6.5e-2 / 6.2e-2, 6.3e-2 / 2.8e-2.
    rows_ref = torch.stack([alpha_ref[b, :, i, :] for b, i in pairs])
    rows_low = torch.stack([alpha_low[b, :, i, :] for b, i in pairs])
    for n, (b, i) in enumerate(pairs):
        print(f'{name} weights of query {(b, i)}: kernel {(res.probs[n] - rows_ref[n]).abs().max().item():.3e} '
              f'eager-same-dtype {(rows_low[n] - rows_ref[n]).abs().max().item():.3e}')
        assert (res.probs[n, :, i + 1:] == 0).all() and (res.contributions[n, :, :, i + 1:] == 0).all()
    _within_2x(res.probs, rows_ref, rows_low, f'{name} weights of the four queries')


def test_the_layer_equals_the_cpu_twin_fed_the_same_operands(hip_model, monkeypatch):
    from src.utils import sense_attribution as SA
    import bp_hip
    name, model, ids = hip_model
    tr = model.transformer
    k = tr.num_content_vectors
    pairs = [(1, 50), (0, S_MODEL - 1), (0, 41)]
    targets = torch.tensor([[7, 99], [4001, 7], [12, 3000]], device=DEV)
    res = SA.sense_contributions(model, ids, pairs, target_ids=targets, return_probs=True)
    with torch.no_grad():
        qk = tr.contextualization_attn.project(tr.gpt2_model(ids))
        table = tr.sense_table()
    assert table is not None
    scale = tr.contextualization_attn.scale()
    qs, qp = torch.tensor([b for b, _ in pairs]), torch.tensor([i for _, i in pairs])
    vec = model.lm_head.weight.detach()[targets].float()
    cpu, cpu_p = SA._eager_sense_attribute(qk.cpu(), table.cpu(), ids.cpu(), qs, qp, vec.cpu(), scale, True)
    want, want_p, unit = R.sense_attribute(qk, table, ids.cpu(), qs, qp, vec, scale)
    # two fp32 evaluations of one contract: each within the first-order bound of the exact value
    factor = 2 * R.fp32_factor(qk, qs, qp, scale, table.shape[2])
    assert (np.abs(res.contributions.double().cpu().numpy() - cpu.double().numpy()) <= factor * unit).all()
    assert (np.abs(res.probs.double().cpu().numpy() - cpu_p.double().numpy()) <= factor * want_p).all()

    # top_contributions: exact on the very contributions the call returned
    for count in (1, 10):
        top = SA.top_contributions(res, count)
        got = (top.top_positions, top.top_senses, top.top_values, top.bottom_positions, top.bottom_senses, top.bottom_values)
        assert (top.top_values[..., -1] > 0).all() and (top.bottom_values[..., -1] < 0).all(), 'no zeros among the extremes'
        for gt, w in zip(got, R.top_contributions(res.contributions.cpu().numpy(), count)):
            assert gt.is_cuda and gt.shape == (3, 2, count)
            if gt.dtype == torch.float32:
                assert (R.bits_of(gt.cpu().numpy()) == R.bits_of(w)).all()
            else:
                assert (gt.cpu().numpy() == w).all()

    # contextual_localize: the HIP path against the same driver with the kernel replaced by the CPU twin
    g = torch.Generator().manual_seed(2)
    contexts = [torch.randint(0, 4096, (n,), generator=g).tolist() for n in (3, 9, 20)]
    contexts[1][2] = contexts[2][4] = contexts[0][0]
    plus, minus = SA.contextual_localize(model, contexts, 77)
    seen = {}

    def twin_call(qk, table, index, qs, qp, vec, scale, want_probs=False, out=None, probs=None):
        o, _ = SA._eager_sense_attribute(qk.cpu(), table.cpu(), index.cpu(), qs.cpu(), qp.cpu(), vec.cpu(), scale)
        seen.update(qk=qk, index=index, qs=qs.cpu(), qp=qp.cpu(), vec=vec)
        out.copy_(o)
        return out, None

    monkeypatch.setattr(bp_hip, 'sense_attribute', twin_call)
    plus_cpu, minus_cpu = SA.contextual_localize(model, contexts, 77)
    monkeypatch.undo()
    assert plus.is_cuda and plus.shape == (model.lm_head.weight.shape[0], k) and not torch.equal(plus, torch.zeros_like(plus))
    _, _, unit = R.sense_attribute(seen['qk'], table, seen['index'].cpu(), seen['qs'], seen['qp'], seen['vec'], scale)
    factor = 2 * R.fp32_factor(seen['qk'], seen['qs'], seen['qp'], scale, table.shape[2])
    allowed = np.zeros((2,) + tuple(plus.shape))
    for n, ctx in enumerate(contexts):
        for j in range(len(ctx) - 1):
            allowed[:, ctx[j], :] += factor * unit[n, :, :, j]
    for nm, a, b, lim in (('plus', plus, plus_cpu, allowed[0]), ('minus', minus, minus_cpu, allowed[1])):
        diff = np.abs(a.double().cpu().numpy() - b.double().cpu().numpy())
        # (+ one fp32 ulp: both results are rounded to fp32 once more when they are returned)
        assert (diff <= lim + _ulp32(b.cpu().numpy())).all(), nm
