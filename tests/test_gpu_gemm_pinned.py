"""GPU: bp_gemm_bf16 / bp_gemm_f16 (csrc/bp_gemm.hip) and the routing helper bp_hip.linear (bp_hip/gemm.py).

a) the entry against an fp64 matmul of the same 16-bit operands, the project's kernel rule: at most 2 x the error of
   torch's own GEMM on those operands plus 1e-5 (docs/DESIGN_NOTES.md section 7) -- odd row counts, N not a multiple of
   the tile, bias / no bias / bias + GELU, both dtypes, a wider output buffer whose guard columns stay intact;
   the tables are test-only ones that pin the heuristic's candidates #0 and, where there is one, #1
b) two calls agree bit for bit, a call on a side stream too
c) every way of not running: unknown shape, another library version, an index the library does not have, a stream that
   is being captured, one row below the M bucket -- nothing is launched and bp_hip.linear is F.linear, bit for bit
d) a Micro model: the shipped table reroutes nothing (logits torch.equal to the plain path), an injected table that pins
   candidate #0 at Micro's shapes stays within the model tests' tolerance, chained == plain LayerNorm path bit for bit
e) one libhipblaslt in the process"""
import pytest
import torch
import torch.nn.functional as F

import bp_hip
from bp_hip import gemm

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ROWS = (1, 255, 256, 257, 1000)
# (K, N, gelu): trunk Wqkv, out_proj, fc2, fc1 + GELU of Backpack-Small, and an N that is no multiple of 256
SHAPES = [(768, 2304, False), (768, 768, False), (3072, 768, False), (768, 3072, True), (768, 520, False)]
NAMES = {torch.bfloat16: 'bf16', torch.float16: 'fp16'}


@pytest.fixture(scope='module')
def here():
    return gemm.library()          # (hipblasLtGetVersion, 'gfx950')


def _table(here, rows):
    """rows: (dtype, epilogue, n, k, m_min, solution)"""
    return bp_hip.GemmTable({'library_version': here[0], 'arch': here[1], 'entries': [
        dict(dtype=NAMES[dt], epilogue=ep, n=n, k=k, m_min=m_min, solution=s) for dt, ep, n, k, m_min, s in rows]})


def _operands(m, k, n, dtype, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.randn(m, k, device=DEV, dtype=dtype, generator=g)
    w = torch.randn(n, k, device=DEV, dtype=dtype, generator=g) * 0.05
    b = torch.randn(n, device=DEV, dtype=dtype, generator=g)
    return x, w, b


def _exact(x, w, b, gelu):
    y = x.double() @ w.double().t()
    if b is not None:
        y = y + b.double()
    return F.gelu(y, approximate='tanh') if gelu else y


def _torch_gemm(x, w, b, gelu):
    return torch._addmm_activation(b, x, w.t(), use_gelu=True) if gelu else F.linear(x, w, b)


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16], ids=['bf16', 'fp16'])
@pytest.mark.parametrize('k, n, gelu', SHAPES, ids=[f'k{k}_n{n}{"_gelu" if g else ""}' for k, n, g in SHAPES])
def test_entry_against_fp64(here, dtype, k, n, gelu):
    ran = 0
    for m in ROWS:
        x, w, b = _operands(m, k, n, dtype, 100 + m)
        for bias in ((b,) if gelu else (None, b)):
            ep = 'none' if bias is None else ('bias_gelu' if gelu else 'bias')
            want = _exact(x, w, bias, gelu)
            base = (_torch_gemm(x, w, bias, gelu).double() - want).abs().max().item()
            picks = gemm.heuristic(dtype, ep, m, n, k, count=2)
            assert picks and picks[0] >= 0, (m, ep)
            for which, solution in enumerate(picks):
                if solution < 0 or (which == 1 and solution == picks[0]):
                    continue
                table = _table(here, [(dtype, ep, n, k, 1, solution)])
                for pad in (0, 24):                     # ldd == N, and rows of a wider buffer
                    buf = torch.full((m, n + pad), 7.0, device=DEV, dtype=dtype)
                    out = buf[:, :n]
                    status = gemm.pinned(x, w, bias, gelu, out, table)
                    if which == 1 and status == 'unsupported':
                        continue                        # a second candidate need not take every problem; #0 must
                    assert status == 'ran', (m, ep, which, solution, status)
                    ran += 1
                    err = (out.double() - want).abs().max().item()
                    print(f'{NAMES[dtype]} m={m} k={k} n={n} {ep} pick#{which}={solution} ldd={n + pad}: err {err:.3e} torch {base:.3e}')
                    assert err <= 2 * base + 1e-5, (m, ep, which, pad, err, base)
                    assert bool((buf[:, n:] == 7.0).all()), 'guard columns written'
                    if pad == 0:
                        # the helper makes this very call into a fresh (M, N) output: the same bound (equal bits of two
                        # calls are test b's subject; which candidates lack them: DESIGN.md section 5)
                        got = bp_hip.linear(x, w, bias, gelu=gelu, table=table)
                        assert got.shape == (m, n) and (got.double() - want).abs().max().item() <= 2 * base + 1e-5
    assert ran >= 2 * len(ROWS)


def test_two_calls_and_a_side_stream_agree_bit_for_bit(here):
    m, k, n = 1000, 768, 2304
    x, w, b = _operands(m, k, n, torch.bfloat16, 5)
    table = _table(here, [(torch.bfloat16, 'bias', n, k, 1, gemm.heuristic(torch.bfloat16, 'bias', m, n, k, count=1)[0])])
    first, second, third = (torch.empty(m, n, device=DEV, dtype=torch.bfloat16) for _ in range(3))
    assert gemm.pinned(x, w, b, False, first, table) == 'ran'
    assert gemm.pinned(x, w, b, False, second, table) == 'ran'
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        assert gemm.pinned(x, w, b, False, third, table) == 'ran'
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert torch.equal(first, second) and torch.equal(first, third)


def test_the_lm_head_row_repeats_its_bits(here):
    """The shape of the one row the shipped table pins (N = 50 264, K = 768, no epilogue) at a modest M: the shipped
    solution (where this process has the library it was measured with) and the heuristic's first candidate each give
    the same bits twice, and stay within the kernel rule."""
    m, k, n = 1000, 768, 50264
    x, w, _ = _operands(m, k, n, torch.bfloat16, 21)
    want = _exact(x, w, None, False)
    base = (F.linear(x, w).double() - want).abs().max().item()
    solutions = [gemm.heuristic(torch.bfloat16, 'none', m, n, k, count=1)[0]]
    shipped = gemm.shipped_table()
    if (shipped.library_version, shipped.arch) == here:
        solutions += [e['solution'] for e in shipped.spec['entries']
                      if e.get('solution') is not None and (e['n'], e['k'], e['epilogue']) == (n, k, 'none')][:1]
    ran = 0
    for solution in dict.fromkeys(solutions):
        table = _table(here, [(torch.bfloat16, 'none', n, k, 1, solution)])
        first, second = (torch.empty(m, n, device=DEV, dtype=torch.bfloat16) for _ in range(2))
        status = gemm.pinned(x, w, None, False, first, table)
        if status == 'unsupported' and solution != solutions[0]:
            continue                      # the row's own bucket starts at 262 144 rows; the first candidate must run
        assert status == 'ran' and gemm.pinned(x, w, None, False, second, table) == 'ran', (solution, status)
        ran += 1
        assert torch.equal(first, second), solution
        assert (first.double() - want).abs().max().item() <= 2 * base + 1e-5, solution
    assert ran >= 1


def test_every_way_of_not_running_is_torch_bit_for_bit(here):
    m, k, n = 257, 768, 768
    x, w, b = _operands(m, k, n, torch.bfloat16, 9)
    want = F.linear(x, w, b)
    pick = gemm.heuristic(torch.bfloat16, 'bias', m, n, k, count=1)[0]
    sentinel = torch.full((m, n), 3.0, device=DEV, dtype=torch.bfloat16)

    def refused(table, status):
        out = sentinel.clone()
        assert gemm.pinned(x, w, b, False, out, table) == status
        assert torch.equal(out, sentinel)                       # nothing was launched
        assert torch.equal(bp_hip.linear(x, w, b, table=table), want)

    refused(bp_hip.GemmTable({}), 'miss')                                                   # no table at all
    refused(_table(here, [(torch.bfloat16, 'bias', n + 8, k, 1, pick)]), 'miss')           # another N
    refused(_table(here, [(torch.bfloat16, 'none', n, k, 1, pick)]), 'miss')               # another epilogue
    refused(_table(here, [(torch.float16, 'bias', n, k, 1, pick)]), 'miss')                # another dtype
    refused(_table((here[0] + 1, here[1]), [(torch.bfloat16, 'bias', n, k, 1, pick)]), 'version')
    refused(_table((here[0], 'gfx942'), [(torch.bfloat16, 'bias', n, k, 1, pick)]), 'version')
    # an index that does not take the problem: the fp16 problem's solution under a bf16 row
    other = gemm.heuristic(torch.float16, 'bias', m, n, k, count=1)[0]
    assert other != pick
    refused(_table(here, [(torch.bfloat16, 'bias', n, k, 1, other)]), 'unsupported')
    # a stream that is being captured: the graph holds torch's GEMM
    good = _table(here, [(torch.bfloat16, 'bias', n, k, 1, pick)])
    assert gemm.pinned(x, w, b, False, sentinel.clone(), good) == 'ran'
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        F.linear(x, w, b)
    torch.cuda.current_stream().wait_stream(side)
    graph, seen = torch.cuda.CUDAGraph(), []
    with torch.cuda.graph(graph):
        seen.append(gemm.pinned(x, w, b, False, sentinel.clone(), good))
        captured = bp_hip.linear(x, w, b, table=good)
    graph.replay()
    torch.cuda.synchronize()
    assert seen == ['capturing'] and torch.equal(captured, want)


def test_a_row_does_not_fire_below_its_m_bucket(here):
    k, n, bucket = 64, 64, 131072
    x, w, b = _operands(bucket, k, n, torch.bfloat16, 13)
    table = _table(here, [(torch.bfloat16, 'bias', n, k, bucket, gemm.heuristic(torch.bfloat16, 'bias', bucket, n, k, count=1)[0])])
    out = torch.full((bucket, n), 3.0, device=DEV, dtype=torch.bfloat16)
    assert gemm.pinned(x[:bucket - 1], w, b, False, out[:bucket - 1], table) == 'miss'
    assert bool((out == 3.0).all())
    assert torch.equal(bp_hip.linear(x[:bucket - 1], w, b, table=table), F.linear(x[:bucket - 1], w, b))
    assert gemm.pinned(x, w, b, False, out, table) == 'ran'
    want = _exact(x, w, b, False)
    base = (F.linear(x, w, b).double() - want).abs().max().item()
    assert (out.double() - want).abs().max().item() <= 2 * base + 1e-5


# ---- d) routing ----------------------------------------------------------------------------------------------------------------

MICRO = dict(n_embd=384, n_head=6, n_layer=6, num_content_vectors=16)


def _micro(**over):
    from src.models.backpack import BackpackConfig, BackpackLMHeadModel
    torch.manual_seed(11)
    kw = dict(vocab_size=50257, n_positions=128, scale_attn_by_inverse_layer_idx=True, resid_pdrop=0.0, embd_pdrop=0.0,
              attn_pdrop=0.0, use_flash_attn=True, fused_bias_fc=True, fused_dense_gelu_dense=True, fused_dropout_add_ln=True,
              pad_vocab_size_multiple=8, dedup_min_positions=1, **MICRO)
    kw.update(over)
    return BackpackLMHeadModel(BackpackConfig(**kw), device=DEV, dtype=torch.bfloat16).eval()


def test_micro_model_routing(here, monkeypatch):
    model = _micro()
    trunk = model.transformer.gpt2_model
    ids = torch.randint(0, 50257, (2, 128), generator=torch.Generator().manual_seed(1)).to(DEV)
    m, d, vocab = ids.numel(), MICRO['n_embd'], 50264
    statuses = []
    inner = gemm.pinned

    def spy(*args):
        statuses.append(inner(*args))
        return statuses[-1]

    monkeypatch.setattr(gemm, 'pinned', spy)
    out = torch.empty(2, 128, vocab, device=DEV, dtype=torch.bfloat16)
    with torch.no_grad():
        # the parent's path: no table at all
        with gemm.use_table(bp_hip.GemmTable({})):
            plain = model(ids).logits
            plain_out = model(ids, logits_out=out).logits.clone()
        assert statuses == []
        # the shipped table: every row starts at 131 072 rows, so nothing here is rerouted
        shipped = model(ids).logits
        assert torch.equal(shipped, plain) and 'ran' not in statuses
        assert torch.equal(model(ids, logits_out=out).logits, plain_out) and 'ran' not in statuses
        # candidate #0 pinned at every dense shape of the whole-batch trunk, the sense projection and the LM head
        bf = torch.bfloat16
        shapes = [('bias', 3 * d, d), ('bias', d, d), ('bias_gelu', 4 * d, d), ('bias', d, 4 * d), ('bias', 2 * d, d),
                  ('none', vocab, d)]
        table = _table(here, [(bf, ep, n, k, 1, gemm.heuristic(bf, ep, m, n, k, count=1)[0]) for ep, n, k in shapes])
        with gemm.use_table(table):
            del statuses[:]
            trunk.ln_chain = True
            chained = model(ids, logits_out=out).logits.clone()
            assert statuses.count('ran') >= 4 * MICRO['n_layer'] + 2, statuses
            trunk.ln_chain = False
            unchained = model(ids, logits_out=out).logits.clone()
            trunk.ln_chain = True
        assert torch.equal(chained, unchained)
    # the model tests' tolerance: 3 x the error of the 16-bit path on torch's GEMMs against an fp32 eager twin, plus 1e-3
    twin = _micro(use_flash_attn=False, fused_bias_fc=False, fused_dense_gelu_dense=False, fused_dropout_add_ln=False)
    twin.load_state_dict(model.state_dict())
    with torch.no_grad():
        want = twin.float()(ids).logits
    err = (chained.float() - want).abs().max().item()
    base = (plain_out.float() - want).abs().max().item()
    print(f'micro logits against the fp32 twin: pinned {err:.3e}, torch GEMMs {base:.3e}')
    assert err <= 3 * base + 1e-3, (err, base)


def test_one_libhipblaslt_in_the_process(here):
    x, w, b = _operands(64, 64, 64, torch.bfloat16, 1)
    table = _table(here, [(torch.bfloat16, 'bias', 64, 64, 1, gemm.heuristic(torch.bfloat16, 'bias', 64, 64, 64, count=1)[0])])
    assert gemm.pinned(x, w, b, False, torch.empty(64, 64, device=DEV, dtype=torch.bfloat16), table) == 'ran'
    F.linear(x, w, b)
    with open('/proc/self/maps') as f:
        paths = {line.split()[-1] for line in f if 'libhipblaslt' in line.rsplit('/', 1)[-1]}
    assert len(paths) == 1, paths
