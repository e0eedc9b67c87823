"""-m gpu: the BASELINE.json configurations at their REAL dimensions (round-1 VERDICT "exercised-config holes"):
config 2 as a whole model (Backpack-Small, S = 1024), config 4's sense kernels at S = 1024 (k = 64, d_k = 10),
config 3's data-parallel wrapper on the ROCm `nccl` backend (= RCCL) with one rank, and the reference's varlen
sweep (tests/test_flash_attn.py:441-461,533-553) on the sequence lengths the fixed-length sweep skips."""
import math
import os

import pytest
import torch

from oracle import ref_cpu as R

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def _bp():
    import bp_hip
    return bp_hip


def _model_from_sd_keys(sd, ocfg, dtype, use_flash, fused):
    """The oracle's state dict lists every tensor once; the module also registers the shared embedding under the
    content model and the position embedding under the trunk only -- build the full key set."""
    from src.models.backpack import BackpackConfig, BackpackLMHeadModel
    cfg = BackpackConfig(n_embd=ocfg['n_embd'], n_head=ocfg['n_head'], n_layer=ocfg['n_layer'],
                         num_content_vectors=ocfg['num_content_vectors'], vocab_size=ocfg['vocab_size'],
                         n_positions=ocfg['n_positions'], scale_attn_by_inverse_layer_idx=True,
                         shrink_final_inner=ocfg.get('shrink_final_inner', False),
                         resid_pdrop=0.0, embd_pdrop=0.0, attn_pdrop=0.0, use_flash_attn=use_flash,
                         fused_dropout_add_ln=fused, fused_dense_gelu_dense=fused, fused_bias_fc=fused,
                         pad_vocab_size_multiple=8)
    model = BackpackLMHeadModel(cfg)
    res = model.load_state_dict(sd, strict=False)
    # shared parameters may be listed under their aliases only
    assert not res.unexpected_keys, res.unexpected_keys
    assert all('embeddings' in k for k in res.missing_keys), res.missing_keys
    model.tie_weights()
    return model.to(DEV, dtype).eval()


_REFERENCE_RUNS = {}


def _oracle_run(name, seq=1024, batch=2):
    """One fp32 CPU oracle forward of `name` at its real size (vocab 50264) plus the HIP-path model and its eager 16-bit
    twin on the GPU, shared by the tests of this module (the Small oracle forward alone is ~20 s of CPU)."""
    if name in _REFERENCE_RUNS:
        return _REFERENCE_RUNS[name]
    ocfg = R.make_config(name, n_positions=seq, vocab_size=50264)
    sd = R.init_state_dict(ocfg, seed=0)
    with torch.no_grad():   # default init gives near-uniform attention; sharpen so the softmax paths matter
        sd['transformer.contextualization_attn.Wqkv.weight'].mul_(8.0)
        for i in range(ocfg['n_layer']):
            sd[f'transformer.gpt2_model.layers.{i}.mixer.Wqkv.weight'].mul_(6.0)
        sd = {k: v.bfloat16().float() for k, v in sd.items()}       # bf16-exact weights for all three runs
    sd['lm_head.weight'] = sd['transformer.gpt2_model.embeddings.word_embeddings.weight']
    ids = torch.randint(0, 50257, (batch, seq), generator=torch.Generator().manual_seed(0))
    with torch.no_grad():
        want = R.backpack_forward(sd, ocfg, ids, return_stages=True)
    want = dict(hidden=want['hidden'], logits=want['logits'])        # (drop alpha: 0.5 GB at k = 64)
    hip = _model_from_sd_keys(sd, ocfg, torch.bfloat16, True, True)
    eager = _model_from_sd_keys(sd, ocfg, torch.bfloat16, False, False)
    with torch.no_grad():
        hid_eager = eager.transformer(ids.to(DEV))
    rows = torch.randint(0, batch * seq, (384,), generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        log_eager = eager.lm_head(hid_eager.flatten(0, 1)[rows.to(DEV)])
    del eager
    run = dict(ocfg=ocfg, ids=ids, want=want, hip=hip, hid_eager=hid_eager, log_eager=log_eager, rows=rows)
    _REFERENCE_RUNS[name] = run
    return run


def _assert_model_parity(run, hid_hip, label):
    """The reference's model-test criterion: err <= 3 x the error of the SAME model in eager bf16 (+1e-3)."""
    rows = run['rows']
    with torch.no_grad():
        log_hip = run['hip'].lm_head(hid_hip.flatten(0, 1)[rows.to(DEV)])
    for got, base, ref, name in ((hid_hip, run['hid_eager'], run['want']['hidden'], 'hidden'),
                                 (log_hip, run['log_eager'], run['want']['logits'].flatten(0, 1)[rows], 'logits')):
        err = (got.float().cpu() - ref).abs().max().item()
        b = (base.float().cpu() - ref).abs().max().item()
        print(f'{label} {name}: hip {err:.3e} eager-bf16 {b:.3e} (|ref| max {ref.abs().max().item():.2f})')
        assert torch.isfinite(got.float()).all()
        assert err <= 3 * b + 1e-3, (label, name, err, b)


def _hidden(run, ids, mode):
    t = run['hip'].transformer
    t.sense_table_mode = mode
    try:
        with torch.no_grad():
            return t(ids.to(DEV))
    finally:
        t.sense_table_mode = 'cached'


def test_small_config2_whole_model_seq1024():
    """BASELINE config 2 as a whole model: Backpack-Small (d 768, 12 heads, 12 layers, k 16, vocab 50264),
    B = 2, S = 1024, bf16, the reference's backpack-small-flash flag set, against the fp32 CPU oracle of the
    reference's eager forward.  Criterion of the reference's model tests: err <= 3 x the error of the SAME
    model in eager bf16 (here the eager twin on the GPU: use_flash_attn / fused flags off).  The content network
    runs on every position, the reference's order of operations (training/src/models/backpack.py:297-314)."""
    run = _oracle_run('small')
    _assert_model_parity(run, _hidden(run, run['ids'], 'off'), 'small S=1024 per position')


@pytest.mark.parametrize('name', ['small', 'mini-k64'])
def test_token_tables_against_the_oracle(name):
    """The two inference orders that run the content network per TOKEN, checked DIRECTLY against the oracle (round-4
    review: the deduplicated path was only compared with the HIP per-position path):
      * the cached whole-vocabulary sense table (the default in eval), B = 2: the oracle's two samples;
      * the table of the batch's distinct tokens (torch.unique), taken from vocab positions up: a batch of
        100 samples whose first two are the oracle's.
    Small's table is 1.2 GB; Mini k = 64's 4.1 GB, i.e. byte offsets beyond 2^31 and up to 96 % of the 32-bit range."""
    run = _oracle_run(name)
    t = run['hip'].transformer
    ids = run['ids']
    hid = _hidden(run, ids, 'cached')
    table = t.sense_table()
    assert table is not None and table.shape == (50264, t.num_content_vectors, run['ocfg']['n_embd'])
    if name == 'mini-k64':
        assert table.numel() * 2 > 2 ** 31 and int(ids.max()) * table.stride(0) * 2 > 2 ** 31
    _assert_model_parity(run, hid, f'{name} cached vocabulary table')
    big = torch.randint(0, 50257, (100, ids.shape[1]), generator=torch.Generator().manual_seed(9))
    big[:2] = ids
    t.sense_table_mode = 'batch'
    with torch.no_grad():
        assert t._dedup_applies(big.to(DEV)) and not t._dedup_applies(big[:48].to(DEV))      # vocab positions up
    hid = _hidden(run, big, 'batch')[:2]
    _assert_model_parity(run, hid, f'{name} table of the distinct tokens of a batch of 100')


def test_mini_k64_config4_whole_model_seq1024():
    """BASELINE config 4 as a whole model at its REAL size (round-4 review): Backpack-Mini, 8 layers, d = 640, 8 heads
    (d_h = 80), k = 64 senses of d_k = 10, `shrink_final_inner` (training/configs/experiment/owt/backpack-mini-flash-vecs-64.yaml),
    vocab 50264, S = 1024, B = 2, bf16, content network per position, against the fp32 CPU oracle; 3 x rule."""
    run = _oracle_run('mini-k64')
    assert run['hip'].transformer.content_model.final_mlp.fc1.weight.shape[0] == 640      # shrink_final_inner
    _assert_model_parity(run, _hidden(run, run['ids'], 'off'), 'mini-k64 S=1024 per position')


@pytest.mark.parametrize('name', ['mini-k4', 'mini-k1'])
def test_mini_few_sense_ablations_whole_model_seq1024(name):
    """The few-sense ends of the reference's sense ablation at their REAL size (training/configs/experiment/owt/
    backpack-mini-flash-vecs-4.yaml: 4 senses of d_k = 160; vecs-1.yaml: one sense of d_k = 640; Mini trunk, vocab 50264,
    S = 1024, B = 2, bf16).  Their sense width lies beyond the narrow LDS-DMA sense kernels (128): since round 6 the ring
    kernels of csrc/sense_wide_dma.hip run them natively (`ContextSelfAttn.fused` True, no warning, no (B,k,S,S) tensor),
    the cached table included: its rows are gathered inside the mix kernel (bp_sense_mix_gather, ABI 9), no torch gather, no
    (B,S,k*d) tensor.  Against the fp32 CPU oracle, 3 x rule, per position and from the cached table."""
    import warnings
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter('always')
        run = _oracle_run(name)
    t = run['hip'].transformer
    assert t.fused_senses and t.use_hip and not any('eager op sequence' in str(w.message) for w in caught)
    assert t.gpt2_model.layers[0].mixer.use_flash_attn
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter('always')
        for mode in ('off', 'cached'):
            _assert_model_parity(run, _hidden(run, run['ids'], mode), f'{name} S=1024 [{mode}]')
    assert t.sense_table_rows() is not None and not any('gathered by torch' in str(w.message) for w in caught)


def test_few_sense_model_trains_on_the_hip_trunk():
    """A training step of a few-sense model (d_k = 160: wide sense kernels forward, alpha-rebuilding backward, HIP trunk,
    fused LayerNorm / dense layers): loss and every parameter's gradient against fp32 autograd of the eager twin (4 x rule
    of the config-3 test)."""
    from src.models.backpack import BackpackConfig, BackpackLMHeadModel
    import warnings
    torch.manual_seed(0)
    kw = dict(n_embd=640, n_head=8, n_layer=2, num_content_vectors=4, vocab_size=1024, n_positions=256,
              scale_attn_by_inverse_layer_idx=True, shrink_final_inner=True, resid_pdrop=0.0, embd_pdrop=0.0,
              attn_pdrop=0.0, pad_vocab_size_multiple=8)
    ref = BackpackLMHeadModel(BackpackConfig(use_flash_attn=False, **kw)).to(DEV).float()
    with torch.no_grad():
        ref.transformer.contextualization_attn.Wqkv.weight.mul_(8.0)
        for layer in ref.transformer.gpt2_model.layers:
            layer.mixer.Wqkv.weight.mul_(6.0)
    sd = ref.state_dict()
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        hip = BackpackLMHeadModel(BackpackConfig(use_flash_attn=True, fused_dropout_add_ln=True, fused_dense_gelu_dense=True,
                                                 fused_bias_fc=True, **kw)).to(DEV).float()
    eager = BackpackLMHeadModel(BackpackConfig(use_flash_attn=False, **kw)).to(DEV).float()
    hip.load_state_dict(sd)
    eager.load_state_dict(sd)
    assert hip.transformer.fused_senses
    ids = torch.randint(0, 1024, (2, 256), device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))
    labels = torch.roll(ids, -1, 1)

    def step(model, autocast):
        model.zero_grad(set_to_none=True)
        with torch.autocast('cuda', dtype=torch.bfloat16, enabled=autocast):
            logits = model(ids).logits
        loss = torch.nn.functional.cross_entropy(logits.float().flatten(0, 1), labels.flatten())
        loss.backward()
        return loss.item(), {n: p.grad.float().clone() for n, p in model.named_parameters() if p.grad is not None}

    l_ref, g_ref = step(ref.train(), False)
    l_hip, g_hip = step(hip.train(), True)
    l_eag, g_eag = step(eager.train(), True)
    assert abs(l_hip - l_ref) <= 4 * abs(l_eag - l_ref) + 1e-3, (l_hip, l_eag, l_ref)
    assert set(g_hip) == set(g_ref)
    for n in g_ref:
        err = (g_hip[n] - g_ref[n]).abs().max().item()
        base = (g_eag[n] - g_ref[n]).abs().max().item()
        assert torch.isfinite(g_hip[n]).all(), n
        assert err <= 4 * base + 1e-4 * max(1.0, g_ref[n].abs().max().item()), (n, err, base)


def test_sense_table_follows_the_weights_and_survives_graph_capture():
    """The cached whole-vocabulary table: equal to the per-position order at B = 1 and B = 4 (up to the BLAS rounding of a
    row when the row count of the content GEMMs changes); rebuilt IN PLACE (same storage) after an in-place weight
    update and after a reload; dropped by .train(); legal under HIP-graph capture, where a replay after
    refresh_inference_caches() sees updated weights."""
    from src.models.backpack import BackpackConfig, BackpackLMHeadModel
    bp = _bp()
    torch.manual_seed(3)
    cfg = BackpackConfig(n_embd=256, n_head=4, n_layer=2, num_content_vectors=8, vocab_size=1000, n_positions=256,
                         scale_attn_by_inverse_layer_idx=True, use_flash_attn=True, fused_dropout_add_ln=True,
                         fused_dense_gelu_dense=True, fused_bias_fc=True, pad_vocab_size_multiple=8)
    model = BackpackLMHeadModel(cfg, device=DEV, dtype=torch.bfloat16).eval()
    t = model.transformer
    with torch.no_grad():
        t.contextualization_attn.Wqkv.weight.mul_(8.0)
    for b in (1, 4):
        ids = torch.randint(0, 1000, (b, 256), device=DEV)
        with torch.no_grad():
            got = t(ids)
            t.sense_table_mode = 'off'
            want = t(ids)
            t.sense_table_mode = 'cached'
        diff = (got.float() - want.float()).abs().max().item()
        assert diff <= 2 ** -7 * want.float().abs().max().item(), (b, diff)
    table = t.sense_table()
    assert table.shape == (1000, 8, 256) and t.sense_table() is table            # kept while nothing changed
    ptr, before = table.data_ptr(), table.clone()
    with torch.no_grad():
        t.content_model.final_mlp.fc2.weight.mul_(2.0)                            # in-place update: _version moves
    after = t.sense_table()
    assert after.data_ptr() == ptr and not torch.equal(after, before)             # refreshed in the SAME storage
    assert (after.float() - 2 * before.float() + t.content_model.final_mlp.fc2.bias.float().view(8, 256)
            ).abs().max().item() < 0.05 * after.float().abs().max().item() + 1e-2
    # graph capture: the replay reads the table's storage, refreshed in front of it
    ids = torch.randint(0, 1000, (2, 256), device=DEV)
    fwd = bp.GraphedForward(model, ids)
    with torch.no_grad():
        assert torch.equal(fwd(ids), model(ids).logits)
        t.content_model.final_mlp.fc2.weight.mul_(0.5)
        assert torch.equal(fwd(ids), model(ids).logits)                           # GraphedForward refreshed the table
    # periodic evaluation during training: the graph pinned the table's storage, so train() / eval() keep the address the
    # captured kernels read; the replay refreshes it in place (advisor, round 5: the table used to be freed here)
    model.train()
    assert t._sense_table.key is None and t._sense_table.rows is not None and t._sense_table.rows.data_ptr() == ptr
    with pytest.raises(RuntimeError):
        fwd(ids)                                                                   # captured in eval mode
    with torch.no_grad():
        t.content_model.final_mlp.fc2.weight.mul_(1.5)                             # "a training step"
    model.eval()
    with torch.no_grad():
        assert torch.equal(fwd(ids), model(ids).logits) and t.sense_table().data_ptr() == ptr
        # weights swapped through `.data` (the reference's EMA, training/src/utils/ema.py:121,165): `_version` does not
        # move.  Bulk forwards check the VALUES (config.sense_table_verify = 'auto': from 16 384 positions up) ...
        t.content_model.final_mlp.fc2.weight.data.mul_(2.0)
        big = torch.randint(0, 1000, (64, 256), device=DEV)
        got = t(big)
        t.sense_table_mode = 'off'
        want = t(big)
        t.sense_table_mode = 'cached'
        assert (got.float() - want.float()).abs().max().item() <= 2 ** -7 * want.float().abs().max().item()
        assert torch.equal(fwd(ids), model(ids).logits)                            # (the rebuild was in place)
        # ... small (latency-bound) ones rely on invalidate_sense_table()
        t.content_model.final_mlp.fc2.weight.data.mul_(0.5)
        stale = t(ids)
        t.invalidate_sense_table()
        fresh = t(ids)
        t.sense_table_mode = 'off'
        want = t(ids)
        t.sense_table_mode = 'cached'
        assert (fresh.float() - want.float()).abs().max().item() <= 2 ** -7 * want.float().abs().max().item()
        assert (stale.float() - want.float()).abs().max().item() > 2 ** -5 * want.float().abs().max().item()
    del fwd
    t.pin_sense_table(False)
    model.train()
    assert t._sense_table.rows is None and t._sense_table.key is None
    model.eval()
    with torch.inference_mode():                                                   # generation runs like this
        out = model(ids).logits
    assert torch.isfinite(out.float()).all() and t.sense_table_rows() is not None


def test_small_config5_whole_model_seq4096_fp16():
    """BASELINE config 5 as a whole model (round-3 review: only the two kernels were checked at S = 4096): Backpack-Small,
    B = 1, S = 4096, fp16, HIP path against the fp32 CPU oracle of the reference's eager forward
    (training/src/models/backpack.py:297-314) on the final hidden states and 256 logit rows; the reference's model-test
    criterion, err <= 3 x the error of the eager fp16 twin on the GPU."""
    seq = 4096
    ocfg = R.make_config('small', n_positions=seq, vocab_size=50264)
    sd = R.init_state_dict(ocfg, seed=0)
    with torch.no_grad():
        sd['transformer.contextualization_attn.Wqkv.weight'].mul_(8.0)
        for i in range(ocfg['n_layer']):
            sd[f'transformer.gpt2_model.layers.{i}.mixer.Wqkv.weight'].mul_(6.0)
        sd = {k: v.half().float() for k, v in sd.items()}           # fp16-exact weights for all three runs
    sd['lm_head.weight'] = sd['transformer.gpt2_model.embeddings.word_embeddings.weight']
    ids = torch.randint(0, 50257, (1, seq), generator=torch.Generator().manual_seed(5))
    with torch.no_grad():
        want = R.backpack_forward(sd, ocfg, ids, return_stages=True)
    hip = _model_from_sd_keys(sd, ocfg, torch.float16, True, True)
    eager = _model_from_sd_keys(sd, ocfg, torch.float16, False, False)
    with torch.no_grad():
        hid_hip = hip.transformer(ids.to(DEV))
        hid_eager = eager.transformer(ids.to(DEV))
        rows = torch.randint(0, seq, (256,), generator=torch.Generator().manual_seed(1))
        rows[:4] = torch.tensor([0, 1, seq - 2, seq - 1])             # both ends of the causal triangle
        log_hip = hip.lm_head(hid_hip.flatten(0, 1)[rows.to(DEV)])
        log_eager = eager.lm_head(hid_eager.flatten(0, 1)[rows.to(DEV)])
    for got, base, ref, name in ((hid_hip, hid_eager, want['hidden'], 'hidden'),
                                 (log_hip, log_eager, want['logits'].flatten(0, 1)[rows], 'logits')):
        err = (got.float().cpu() - ref).abs().max().item()
        b = (base.float().cpu() - ref).abs().max().item()
        print(f'small S=4096 fp16 {name}: hip {err:.3e} eager-fp16 {b:.3e} (|ref| max {ref.abs().max().item():.2f})')
        assert torch.isfinite(got.float()).all()
        assert err <= 3 * b + 1e-3, (name, err, b)


def test_mini_k64_config4_sense_kernels_seq1024():
    """BASELINE config 4 at its real sequence length: k = 64 senses of d_k = 10 (zero-padded to 16 by
    ContextSelfAttn.project), d = 640, S = 1024.  LSE, alpha (row sums, exact zeros above the diagonal, a row
    subset against the oracle) and the fused mix on a row subset."""
    bp = _bp()
    from src.models.backpack import ContextSelfAttn
    torch.manual_seed(7)
    b, s, k, d = 2, 1024, 64, 640
    attn = ContextSelfAttn(k, d, use_hip=True).to(DEV, torch.bfloat16)
    with torch.no_grad():
        attn.Wqkv.weight.mul_(40.0)
    h = torch.randn(b, s, d, device=DEV, dtype=torch.bfloat16)
    c = torch.randn(b, s, k, d, device=DEV, dtype=torch.bfloat16)
    with torch.no_grad():
        qk = attn.project(h)
        assert qk.shape == (b, s, 2, k, 16) and torch.count_nonzero(qk[..., 10:]) == 0
        scale = attn.scale()
        assert abs(scale - 10 ** -0.5) < 1e-12
        lse = bp.sense_lse(qk, scale)
        alpha = bp.sense_alpha(qk, scale, lse=lse)
        out = bp.sense_mix(qk, c, scale, lse=lse)
    rows = torch.tensor([0, 1, 31, 32, 63, 64, 255, 256, 257, 511, 512, 1000, 1023])
    q32, k32 = qk[:, :, 0, :, :10].float().cpu(), qk[:, :, 1, :, :10].float().cpu()
    scores = torch.einsum('btld,bsld->blts', q32[:, rows], k32) * scale          # (b, k, rows, S)
    dead = torch.arange(s)[None, :] > rows[:, None]
    scores = scores.masked_fill(dead[None, None], float('-inf'))
    want_lse = torch.logsumexp(scores, -1)
    want_alpha = torch.softmax(scores, -1)
    assert (lse[:, :, rows].cpu() - want_lse).abs().max().item() < 2e-3
    assert (alpha[:, :, rows].float().cpu() - want_alpha).abs().max().item() < 4e-3
    # size-independent properties on the whole tensor: rows sum to 1, exact zeros above the diagonal
    assert (alpha.float().sum(-1) - 1).abs().max().item() < 2e-2
    upper = torch.ones(s, s, dtype=torch.bool, device=DEV).triu(1)
    assert torch.count_nonzero(alpha[:, :, upper]) == 0
    want = torch.einsum('blts,bsld->btd', want_alpha, c.float().cpu())
    got = out[:, rows].float().cpu()
    # eager bf16 yardstick: the reference's op sequence (alpha rounded to bf16, per-sense bf16 matmul, bf16 sum)
    eager = torch.sum(want_alpha.bfloat16() @ c.cpu().transpose(1, 2), dim=1).float()
    err, base = (got - want).abs().max().item(), (eager - want).abs().max().item()
    print(f'mini-k64 S=1024 mix rows: hip {err:.3e} eager-bf16 {base:.3e}')
    assert err <= 2 * base + 1e-5


def test_ddp_on_nccl_world1_equals_plain_backward():
    """BASELINE config 3's wrapper on the GPU: torch DDP on the ROCm `nccl` backend (= RCCL) with the
    reference's flags (training/src/train.py:97-102: find_unused_parameters=False,
    gradient_as_bucket_view=True), world size 1 on the leased GPU.  RCCL is loaded, the bucket hooks run over the
    custom autograd Functions (flash, sense mix, fused LayerNorm, fused CE), and the all-reduced gradients equal
    those of the unwrapped model bit for bit."""
    import torch.distributed as dist
    from torch.nn.parallel import DistributedDataParallel as DDP
    from flash_attn.losses.cross_entropy import CrossEntropyLoss
    from src.models.backpack import BackpackConfig, BackpackLMHeadModel
    if dist.is_initialized():
        dist.destroy_process_group()
    os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
    os.environ.setdefault('MASTER_PORT', '29531')
    os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
    dist.init_process_group('nccl', rank=0, world_size=1, device_id=torch.device('cuda', 0))
    try:
        kw = dict(n_embd=128, n_head=2, n_layer=2, num_content_vectors=4, vocab_size=512, n_positions=128,
                  scale_attn_by_inverse_layer_idx=True, resid_pdrop=0.0, embd_pdrop=0.0, attn_pdrop=0.0,
                  pad_vocab_size_multiple=8, use_flash_attn=True, fused_dropout_add_ln=True)
        torch.manual_seed(3)
        plain = BackpackLMHeadModel(BackpackConfig(**kw)).to(DEV, torch.bfloat16)
        wrapped = BackpackLMHeadModel(BackpackConfig(**kw)).to(DEV, torch.bfloat16)
        wrapped.load_state_dict(plain.state_dict())
        ddp = DDP(wrapped, device_ids=[0], find_unused_parameters=False, gradient_as_bucket_view=True)
        ids = torch.randint(0, 512, (4, 128), device=DEV)
        labels = torch.randint(0, 512, (4 * 128,), device=DEV)
        loss_fn = CrossEntropyLoss()
        for m in (plain, ddp):
            loss = loss_fn(m(ids).logits.flatten(0, 1), labels)
            loss.backward()
        t = torch.ones(8, device=DEV)
        dist.all_reduce(t)                         # one explicit RCCL collective as well
        torch.cuda.synchronize()
        assert torch.equal(t, torch.ones(8, device=DEV))
        n = 0
        for (name, p), (_, q) in zip(plain.named_parameters(), wrapped.named_parameters()):
            assert p.grad is not None and q.grad is not None, name
            assert torch.equal(p.grad, q.grad), name
            n += 1
        assert n > 20
    finally:
        dist.destroy_process_group()


def _random_padding_mask(max_len, batch, mode, gen):
    """The reference's generate_random_padding_mask (tests/test_flash_attn.py:25-40)."""
    if mode == 'full':
        lengths = torch.full((batch,), max_len)
    elif mode == 'random':
        lengths = torch.randint(max(1, max_len - 20), max_len + 1, (batch,), generator=gen)
    else:   # 'third'
        lengths = torch.randint(max_len // 3, max_len + 1, (batch,), generator=gen)
    return torch.arange(max_len)[None, :] < lengths[:, None]


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16])
@pytest.mark.parametrize('causal', [False, True])
@pytest.mark.parametrize('d', [128, 64, 80, 40, 32, 16])
@pytest.mark.parametrize('seqlen', [113, 384, 512, 768, 1025, 2048])
def test_flash_varlen_sweep(seqlen, d, causal, dtype):
    """The reference's test_flash_attn_unpadded_qkvpacked sweep (random key-padding masks, its head dims and
    sequence lengths, tests/test_flash_attn.py:350-373 with dropout 0) through unpad_input ->
    flash_attn_unpadded_qkvpacked_func -> pad_input, forward and backward: 2x (fwd) / 4x (bwd) the eager
    same-dtype error against the fp32 oracle, the reference's own bounds (:424-437)."""
    from flash_attn.bert_padding import pad_input, unpad_input
    from flash_attn.flash_attn_interface import flash_attn_unpadded_qkvpacked_func
    gen = torch.Generator().manual_seed(seqlen * 131 + d)
    batch, h = (2, 2) if seqlen >= 1025 else (4, 3)
    mode = ('random', 'third', 'full')[(seqlen + d) % 3]
    x = torch.randn(batch, seqlen, 3, h, d, generator=gen).to(dtype)
    mask = _random_padding_mask(seqlen, batch, mode, gen)
    qkv = x.to(DEV).requires_grad_()
    rows, indices, cu, max_len = unpad_input(qkv.flatten(2), mask.to(DEV))
    out_unpad = flash_attn_unpadded_qkvpacked_func(rows.unflatten(-1, (3, h, d)), cu, max_len, 0.0, causal=causal)
    out = pad_input(out_unpad.flatten(1), indices, batch, seqlen).unflatten(-1, (h, d))
    g = torch.randn(batch, seqlen, h, d, generator=gen).to(dtype)
    dqkv, = torch.autograd.grad(out, qkv, g.to(DEV))

    def oracle(upcast, reorder):
        t = x.clone().requires_grad_()
        o = R.attention_fp32(t[:, :, 0], t[:, :, 1], t[:, :, 2], causal=causal, query_padding_mask=mask,
                             key_padding_mask=mask, upcast=upcast, reorder_ops=reorder)[0]
        go, = torch.autograd.grad(o, t, g)
        go = go.masked_fill(~mask[:, :, None, None, None], 0.0)
        return o.detach(), go

    o32, g32 = oracle(True, False)
    o16, g16 = oracle(False, True)
    err, base = (out.float().cpu() - o32.float()).abs().max().item(), (o16.float() - o32.float()).abs().max().item()
    assert err <= 2 * base + 1e-5, ('out', err, base)
    gerr, gbase = (dqkv.float().cpu() - g32.float()).abs().max().item(), (g16.float() - g32.float()).abs().max().item()
    assert gerr <= 4 * gbase + 1e-4, ('dqkv', gerr, gbase)
    # padded rows: zero output, zero gradient (bit-exact)
    assert torch.count_nonzero(out[~mask.to(DEV)]) == 0 and torch.count_nonzero(dqkv[~mask.to(DEV)]) == 0


# ---------------------------------------------------------------------------------------------------------------
# BASELINE config 3 readiness on ONE GPU: the per-GPU training workload at its real dimensions, and the launch path
# ---------------------------------------------------------------------------------------------------------------
def test_small_config3_training_step_seq1024():
    """Config 3's per-GPU workload: Backpack-Small, S = 1024, the reference's recipe (fp32 parameters under bf16
    autocast, training/configs/trainer/default.yaml precision 16), dropout 0, ONE forward + fused cross-entropy +
    backward through all 12 layers of flash-bwd / LayerNorm-bwd / fused dense / sense-mix-bwd.  Loss and the gradients
    of ten named parameters against fp32 autograd of the eager twin (use_flash_attn and every fused flag off, fp32, no
    autocast); criterion of the reference's gradient tests (tests/test_flash_attn.py:435-437): error <= 4 x the
    error of the eager twin under the same bf16 autocast."""
    from flash_attn.losses.cross_entropy import CrossEntropyLoss
    from src.models.backpack import BackpackConfig, BackpackLMHeadModel
    kw = dict(n_embd=768, n_head=12, n_layer=12, num_content_vectors=16, vocab_size=50257, n_positions=1024,
              scale_attn_by_inverse_layer_idx=True, resid_pdrop=0.0, embd_pdrop=0.0, attn_pdrop=0.0,
              pad_vocab_size_multiple=8)
    torch.manual_seed(21)
    eager = BackpackLMHeadModel(BackpackConfig(use_flash_attn=False, **kw), device=DEV).train()
    with torch.no_grad():   # default init gives near-uniform attention; sharpen so the softmax backward matters
        eager.transformer.contextualization_attn.Wqkv.weight.mul_(8.0)
        for layer in eager.transformer.gpt2_model.layers:
            layer.mixer.Wqkv.weight.mul_(6.0)
    hip = BackpackLMHeadModel(BackpackConfig(use_flash_attn=True, fused_dropout_add_ln=True, fused_bias_fc=True,
                                             fused_dense_gelu_dense=True, **kw), device=DEV).train()
    hip.load_state_dict(eager.state_dict())
    ids = torch.randint(0, 50257, (1, 1024), device=DEV, generator=torch.Generator(device=DEV).manual_seed(0))
    labels = torch.roll(ids, -1, 1).reshape(-1)
    names = ['transformer.gpt2_model.layers.0.mixer.Wqkv.weight', 'transformer.gpt2_model.layers.11.mixer.Wqkv.weight',
             'transformer.gpt2_model.layers.5.mixer.out_proj.bias', 'transformer.gpt2_model.layers.3.mlp.fc1.bias',
             'transformer.gpt2_model.layers.7.mlp.fc2.weight', 'transformer.contextualization_attn.Wqkv.weight',
             'transformer.contextualization_attn.Wqkv.bias', 'transformer.content_model.final_mlp.fc2.weight',
             'transformer.content_model.final_mlp.fc1.bias', 'transformer.gpt2_model.embeddings.word_embeddings.weight',
             'transformer.gpt2_model.layers.6.norm1.weight', 'transformer.gpt2_model.embeddings.position_embeddings.weight']

    def run(model, autocast, fused_loss):
        model.zero_grad(set_to_none=True)
        with torch.autocast('cuda', dtype=torch.bfloat16, enabled=autocast):
            logits = model(ids).logits
        flat = logits.reshape(-1, logits.shape[-1])
        loss = CrossEntropyLoss()(flat, labels) if fused_loss else torch.nn.functional.cross_entropy(flat.float(), labels)
        loss.backward()
        params = dict(model.named_parameters())
        return loss.item(), {n: params[n].grad.detach().float().cpu() for n in names}

    l_ref, g_ref = run(eager, False, False)
    l_low, g_low = run(eager, True, False)
    eager.zero_grad(set_to_none=True)
    l_hip, g_hip = run(hip, True, True)
    print(f'config-3 step: loss fp32 {l_ref:.5f} eager-amp {l_low:.5f} hip-amp {l_hip:.5f}')
    assert abs(l_hip - l_ref) <= 4 * abs(l_low - l_ref) + 5e-3
    for n in names:
        r = g_ref[n]
        err, base = (g_hip[n] - r).abs().max().item(), (g_low[n] - r).abs().max().item()
        scale = r.abs().max().item()
        print(f'  {n}: hip {err:.3e} eager-amp {base:.3e} |ref| {scale:.3e}')
        assert torch.isfinite(g_hip[n]).all() and scale > 0, n
        assert err <= 4 * base + 1e-3 * scale, (n, err, base, scale)
    for p in hip.parameters():
        assert p.grad is not None and p.grad.dtype == torch.float32


def _torchrun(script_args, timeout=900):
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY='0')
    for k in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT'):
        env.pop(k, None)
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '1', '--master-addr',
           '127.0.0.1', '--master-port', '29533'] + script_args
    r = subprocess.run(cmd, cwd=root, env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    import json
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_bench_launch_path_under_torchrun():
    """The driver's N-GPU launch line with N = 1: `python -m torch.distributed.run ... bench.py --gpus 1` goes through
    init_process_group('nccl'), the batch broadcast, the barriers and the MAX all-reduce of the elapsed time -- the code
    the 8-GPU run depends on -- and prints ONE JSON line with the contract's fields."""
    line = _torchrun(['bench.py', '--gpus', '1', '--steps', '2', '--warmup', '1', '--batch', '8', '--no-cpu-baseline', '--full'])
    assert line['n_gpus'] == 1 and line['steps'] == 2 and line['unit'] == 'tokens/s' and line['value'] > 0
    assert line['config']['batch_per_gpu'] == 8 and line['scaling'] == 'weak' and 'roofline' in line
    line = _torchrun(['bench.py', '--gpus', '1', '--steps', '1', '--warmup', '1', '--batch', 'auto', '--batch-candidates',
                      '4,8', '--no-cpu-baseline'])
    assert line['config']['batch_per_gpu'] in (4, 8) and len(line['batch_sweep']) == 2


def test_train_step_launch_path_under_torchrun():
    """scripts/bench_train_step.py the same way: DDP over nccl (RCCL) with the reference's flags, one rank."""
    line = _torchrun(['scripts/bench_train_step.py', '--batch', '2', '--steps', '1', '--warmup', '1'])
    assert line['n_gpus'] == 1 and line['value'] > 0 and line['launch'].startswith('torch.distributed.run')
    assert line['grad_allreduce_bytes'] > 680e6 and line['loss'] > 0
