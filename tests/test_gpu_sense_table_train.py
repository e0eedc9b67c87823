"""GPU: training with the content network once per distinct token -- bp_hip.SenseMixGatherFn (the sense mix over a table of
rows with a backward: bp_sense_mix_dc, bp_segment_sum_rows, the slab backward on a gathered chunk) against SenseMixFn on the
torch-gathered content, against the fp32 oracle's autograd, its memory, its reruns, and the whole model with
config.sense_table_train='batch'."""
import warnings

import pytest
import torch

from decode_support import DEV, _bp
from oracle import ref_cpu as R

pytestmark = pytest.mark.gpu

SHAPES = [(2, 200, 16, 48, 768, 37), (1, 96, 4, 24, 104, 5)]      # (B, S, k, d_k, d, U)


def _inputs(shape, seed=21):
    b, s, k, dk, d, u = shape
    gen = torch.Generator().manual_seed(seed)
    qk = (torch.randn(b, s, 2, k, dk, generator=gen) * 1.2).bfloat16()
    table = torch.randn(u, k, d, generator=gen).bfloat16()
    index = torch.randint(0, u, (b, s), generator=gen)
    index[0, :u] = torch.randperm(u, generator=gen)               # every row is read
    dout = torch.randn(b, s, d, generator=gen).bfloat16()
    return qk, table, index, dout


def _table_grads(bp, qk, table, index, dout, chunk_samples):
    qk, table = qk.to(DEV).requires_grad_(), table.to(DEV).requires_grad_()
    out = bp.sense_mix_gather_autograd(qk, table, index.to(DEV), None, chunk_samples=chunk_samples)
    assert out.grad_fn is not None and type(out.grad_fn).__name__.startswith('SenseMixGatherFn')
    return out, torch.autograd.grad(out, (qk, table), dout.to(DEV))


def _oracle_grads(qk, table, index, dout, dtype):
    """dqk and dtable of the oracle's ops on the gathered rows, by autograd in `dtype` on the CPU."""
    q_, t_ = qk.to(dtype).clone().requires_grad_(), table.to(dtype).clone().requires_grad_()
    content = torch.nn.functional.embedding(index, t_.view(t_.shape[0], -1)).view(*index.shape, *t_.shape[1:])
    out = R.sense_mix(R.sense_alpha_from_qk(q_), content.transpose(1, 2))
    return torch.autograd.grad(out, (q_, t_), dout.to(out.dtype))


@pytest.mark.parametrize('shape', SHAPES)
def test_table_form_against_the_dense_form_on_gathered_content(shape):
    """chunk_samples >= B: the two backwards issue the same launches on the same bits for dqk (torch.equal); dtable is the
    float64 index-add of the dense form's dcontent within the bound of an fp32 sum (n 2^-24 sum|x|) plus one rounding to
    bf16 (8 significant bits: 2^-8 relative)."""
    bp = _bp()
    b, s, k, dk, d, u = shape
    qk, table, index, dout = _inputs(shape)
    out, (dqk, dtable) = _table_grads(bp, qk, table, index, dout, chunk_samples=max(b, 8))
    qk_d = qk.to(DEV).requires_grad_()
    content = torch.nn.functional.embedding(index.to(DEV), table.to(DEV).view(u, -1)).view(b, s, k, d).requires_grad_()
    dense = bp.sense_mix_autograd(qk_d, content, None)
    assert bp._fused_mix_backward_ok(qk_d, content, None)
    dqk_dense, dcontent = torch.autograd.grad(dense, (qk_d, content), dout.to(DEV))
    assert torch.equal(dqk, dqk_dense)
    flat = dcontent.double().cpu().view(b * s, k * d)
    exact = torch.zeros(u, k * d, dtype=torch.float64).index_add_(0, index.view(-1), flat)
    magnitude = torch.zeros(u, k * d, dtype=torch.float64).index_add_(0, index.view(-1), flat.abs())
    n = torch.bincount(index.view(-1), minlength=u).double()[:, None]
    bound = n * 2.0 ** -24 * magnitude
    bound = bound + 2.0 ** -8 * (exact.abs() + bound)
    err = (dtable.double().cpu().view(u, k * d) - exact).abs()
    print(f'dtable {shape}: max err {err.max().item():.3e}, max err / bound {(err / bound.clamp_min(1e-300)).max().item():.3f}')
    assert dtable.shape == table.shape and dtable.dtype == table.dtype
    assert (err <= bound).all()


@pytest.mark.parametrize('shape', SHAPES)
def test_one_sample_chunks_against_the_fp32_oracle(shape):
    """chunk_samples = 1 (as many chunks as samples, dtable accumulated over them): dqk and dtable against fp32 autograd of
    the oracle with the rule of test_sense_mix_backward, err <= 2 base + 1e-3 max(1, |ref| max), base the eager-bf16 error."""
    bp = _bp()
    qk, table, index, dout = _inputs(shape)
    ref = _oracle_grads(qk, table, index, dout, torch.float32)
    eager = _oracle_grads(qk, table, index, dout, torch.bfloat16)
    _, got = _table_grads(bp, qk, table, index, dout, chunk_samples=1)
    for g, r, e, name in zip(got, ref, eager, ('dqk', 'dtable')):
        err = (g.float().cpu() - r).abs().max().item()
        base = (e.float() - r).abs().max().item()
        print(f'table mix bwd {shape} {name}: hip {err:.3e} eager {base:.3e}')
        assert g.shape == r.shape and torch.isfinite(g.float()).all()
        assert err <= 2 * base + 1e-3 * max(1.0, r.abs().max().item()), (name, err, base)
    # a rerun of the backward is bit-equal: no atomics anywhere, the chunks are added in ascending order
    _, again = _table_grads(bp, qk, table, index, dout, chunk_samples=1)
    assert torch.equal(again[0], got[0]) and torch.equal(again[1], got[1])


def test_backward_allocates_no_batch_sized_content():
    """Peak memory of the backward at (4, 512, 16, 48, 768) with one-sample chunks: below outputs + the fp32 table + two
    one-sample chunk buffers + one one-sample slab + 8 MB -- which is below ONE (B, S, k, d) tensor."""
    bp = _bp()
    shape = (4, 512, 16, 48, 768, 100)
    b, s, k, dk, d, u = shape
    qk, table, index, dout = _inputs(shape)
    qk_d, table_d, dout_d = qk.to(DEV).requires_grad_(), table.to(DEV).requires_grad_(), dout.to(DEV)
    out = bp.sense_mix_gather_autograd(qk_d, table_d, index.to(DEV), None, chunk_samples=1)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    got = torch.autograd.grad(out, (qk_d, table_d), dout_d)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    outputs = qk.numel() * 2 + table.numel() * 2
    chunk, slab = s * k * d * 2, s * k * bp.SLAB * 2
    allowed = outputs + table.numel() * 4 + 2 * chunk + slab + (8 << 20)
    print(f'table mix bwd {shape}: peak {peak / 2**20:.1f} MiB, allowed {allowed / 2**20:.1f} MiB, '
          f'a (B,S,k,d) tensor {b * chunk / 2**20:.1f} MiB')
    assert peak <= allowed
    assert allowed < b * chunk
    assert all(torch.isfinite(g.float()).all() for g in got)


def test_autograd_refuses_what_the_fused_route_does_not_take():
    bp = _bp()
    qk = torch.zeros(1, 64, 2, 2, 160, dtype=torch.bfloat16, device=DEV, requires_grad=True)
    table = torch.zeros(5, 2, 64, dtype=torch.bfloat16, device=DEV)
    index = torch.zeros(1, 64, dtype=torch.int64, device=DEV)
    assert not bp.sense_mix_gather_train_supported(qk, table, 64)
    with pytest.raises(RuntimeError, match='128'):
        bp.sense_mix_gather_autograd(qk, table, index)
    with torch.no_grad():       # the plain kernel takes it
        assert bp.sense_mix_gather_autograd(qk, table, index).shape == (1, 64, 64)


# ---- the whole model ------------------------------------------------------------------------------------------------------------

def _ids(batch, seqlen, vocab, distinct=20):
    gen = torch.Generator().manual_seed(3)
    tokens = torch.randperm(vocab, generator=gen)[:distinct]
    return tokens[torch.randint(0, distinct, (batch, seqlen), generator=gen)]


def test_backpack_training_step_in_the_table_order():
    """The configuration and the three models of test_backpack_training_step_on_the_hip_path (fp32 CPU reference, bf16 CPU
    eager, bf16 HIP), the HIP model with sense_table_train='batch', ids drawn from 20 distinct tokens; that test's margins."""
    from flash_attn.losses.cross_entropy import CrossEntropyLoss
    from src.models.backpack import BackpackConfig, BackpackLMHeadModel
    kw = dict(n_embd=128, n_head=2, n_layer=2, num_content_vectors=4, vocab_size=512, n_positions=64,
              scale_attn_by_inverse_layer_idx=True, resid_pdrop=0.0, embd_pdrop=0.0, attn_pdrop=0.0,
              pad_vocab_size_multiple=8)
    torch.manual_seed(13)
    ref = BackpackLMHeadModel(BackpackConfig(use_flash_attn=False, **kw)).train()
    with torch.no_grad():
        ref.transformer.contextualization_attn.Wqkv.weight.mul_(6.0)
    hip = BackpackLMHeadModel(BackpackConfig(use_flash_attn=True, fused_dropout_add_ln=True, fused_bias_fc=True,
                                             fused_dense_gelu_dense=True, sense_table_train='batch', **kw)).train()
    hip.load_state_dict(ref.state_dict())
    hip = hip.to(DEV, torch.bfloat16)
    low = BackpackLMHeadModel(BackpackConfig(use_flash_attn=False, **kw)).train()
    low.load_state_dict(ref.state_dict())
    low = low.to(torch.bfloat16)
    ids = _ids(3, 64, 512)
    labels = torch.roll(ids, -1, 1)
    seen = []
    hip.transformer.content_model.register_forward_hook(lambda mod, args, out: seen.append(tuple(args[0].shape)))

    def step(model, x, y, fused_loss):
        logits = model(x).logits
        flat = logits.reshape(-1, logits.shape[-1])
        if fused_loss:
            loss = CrossEntropyLoss()(flat, y.reshape(-1))
        else:
            loss = torch.nn.functional.cross_entropy(flat.float(), y.reshape(-1))
        loss.backward()
        return loss.item()

    l_ref = step(ref, ids, labels, False)
    l_low = step(low, ids, labels, False)
    with warnings.catch_warnings(record=True) as said:
        warnings.simplefilter('always')
        l_hip = step(hip, ids.to(DEV), labels.to(DEV), True)
    assert not [w for w in said if 'sense_table_train' in str(w.message)]      # no fallback, no dropout caveat here
    assert seen == [(1, 20)]                    # the content network saw U rows, not B * S
    assert abs(l_hip - l_ref) <= 3 * abs(l_low - l_ref) + 2e-2
    worst = 0.0
    for (name, p_ref), p_low, p_hip in zip(ref.named_parameters(), low.parameters(), hip.parameters()):
        assert p_hip.grad is not None, name
        r = p_ref.grad
        err = (p_hip.grad.float().cpu() - r).abs().max().item()
        base = (p_low.grad.float() - r).abs().max().item()
        scale = max(r.abs().max().item(), 1e-6)
        worst = max(worst, err / scale)
        assert err <= 4 * base + 2e-2 * scale, (name, err, base, scale)
    print('training step, table order: loss', l_ref, l_hip, 'worst relative grad error', worst)
    # eval() and no_grad forwards of the same model take the inference routes as before
    seen.clear()
    with torch.no_grad():
        hip(ids.to(DEV))
    assert seen == [(3, 64)]                    # train() mode without gradients: per position, as without the option


def test_wide_senses_train_per_position_and_say_so_once():
    from src.models.backpack import BackpackConfig, BackpackLMHeadModel
    torch.manual_seed(2)
    cfg = BackpackConfig(n_embd=320, n_head=5, n_layer=1, num_content_vectors=2, vocab_size=512, n_positions=64,
                         resid_pdrop=0.0, embd_pdrop=0.0, attn_pdrop=0.0, pad_vocab_size_multiple=8, use_flash_attn=True,
                         sense_table_train='batch')
    model = BackpackLMHeadModel(cfg).to(DEV, torch.bfloat16).train()
    ids = _ids(2, 64, 512).to(DEV)
    seen = []
    model.transformer.content_model.register_forward_hook(lambda mod, args, out: seen.append(tuple(args[0].shape)))
    with warnings.catch_warnings(record=True) as said:
        warnings.simplefilter('always')
        for _ in range(2):
            model(ids).logits.float().square().mean().backward()
    said = [w for w in said if 'sense_table_train' in str(w.message)]
    assert len(said) == 1 and '> 128' in str(said[0].message) and 'per position' in str(said[0].message)
    assert seen == [(2, 64), (2, 64)]
    assert all(p.grad is not None and torch.isfinite(p.grad.float()).all() for p in model.parameters())
