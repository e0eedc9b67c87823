"""GPU: src/utils/sense_vocab.py on the HIP path (bp_row_extremes behind `_project_rows`) in bf16 and fp16, on the nano
configuration with a chunk size that leaves a partial last chunk.

  non_contextual_localize  against the float64 restatement (tests/sense_vocab_ref.py) fed the model's own rounded sense
                           vectors and embedding, every score within twice the first-order bound of localize_bound
  sense_extremes           ids and logits against the restatement applied to the very logits blocks the driver produced:
                           exact
  memory                   one whole-vocabulary call at 50 264 vocabulary rows, k = 4: the peak above what was allocated
                           before the call is the reused block plus the outputs, never a (V k, V) matrix"""
import numpy as np
import pytest
import torch

import sense_vocab_ref as R
from decode_support import DEV, _bp

pytestmark = pytest.mark.gpu

DTYPES = {'bf16': torch.bfloat16, 'fp16': torch.float16}
VOCAB, K, D = 96, 4, 64
CHUNK = 100                      # 384 rows: three full chunks and one of 84


def _model(dtype, vocab=VOCAB, n_layer=2):
    import warnings
    from src.models.backpack import BackpackConfig, BackpackLMHeadModel
    torch.manual_seed(7)
    cfg = BackpackConfig(n_embd=D, n_head=2, n_layer=n_layer, num_content_vectors=K, vocab_size=vocab, n_positions=32,
                         scale_attn_by_inverse_layer_idx=True, resid_pdrop=0.0, embd_pdrop=0.0, attn_pdrop=0.0,
                         use_flash_attn=True, pad_vocab_size_multiple=8)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        return BackpackLMHeadModel(cfg).to(DEV, dtype).eval()


@pytest.fixture(scope='module', params=sorted(DTYPES))
def nano(request):
    _bp()
    model = _model(DTYPES[request.param])
    table = model.transformer.sense_table()
    assert table is not None and table.shape == (VOCAB, K, D) and table.dtype == DTYPES[request.param]
    target = torch.zeros(VOCAB)
    target[[3, 17, 40, 95]] = 1.0
    return request.param, model, table.double().cpu().numpy(), model.lm_head.weight.detach().double().cpu().numpy(), target


def test_localize_stays_within_the_first_order_bound(nano):
    from src.utils import sense_vocab as SV
    name, model, senses, emb, target = nano
    want = R.non_contextual_localize(senses, emb, target.numpy())
    bound = 2 * R.localize_bound(senses, emb, target.numpy(), DTYPES[name])
    got = SV.non_contextual_localize(target.to(DEV), model, chunk_rows=CHUNK)
    assert got.shape == (VOCAB, K) and got.dtype == torch.float32 and got.is_cuda
    err = np.abs(got.double().cpu().numpy() - want)
    print(f'localize {name} hip: largest error / allowed = {(err / bound).max():.3f}; '
          f'largest relative error {np.max(err / np.abs(want)):.2e}')
    assert (err <= bound).all()
    zeroed = SV.non_contextual_localize(target, model, chunk_rows=CHUNK, last_token_id=90)
    assert (zeroed[90:] == 0).all() and torch.equal(zeroed[:90], got[:90])


def test_sense_extremes_are_exact_on_the_blocks_the_driver_produced(nano):
    from src.utils import sense_vocab as SV
    name, model, senses, emb, _ = nano
    for count in (1, 6, 64):
        res, blocks = SV.sense_extremes(model, count=count, chunk_rows=CHUNK, _debug_blocks=True)
        assert [b.shape[0] for b in blocks] == [100, 100, 100, 84] and all(b.dtype == DTYPES[name] for b in blocks)
        tv, ti, bv, bi = R.row_extremes(torch.cat(blocks), count)
        shape = (VOCAB, K, count)
        assert res.top_ids.dtype == torch.int64 and res.top_ids.shape == shape
        assert (res.top_ids.cpu().numpy() == ti.reshape(shape)).all() and (res.bottom_ids.cpu().numpy() == bi.reshape(shape)).all()
        assert (R.bits_of(res.top_logits.cpu().numpy()) == R.bits_of(tv.reshape(shape))).all()
        assert (R.bits_of(res.bottom_logits.cpu().numpy()) == R.bits_of(bv.reshape(shape))).all()
    # the blocks are the product they claim to be: the fp32 product of the same rounded operands, to the dtype's rounding
    exact = torch.from_numpy(senses.reshape(-1, D) @ emb.T)
    torch.testing.assert_close(torch.cat(blocks).double().cpu(), exact, rtol=2 * R.EPS_OUT[DTYPES[name]], atol=1e-4)
    rows = [5, 17, 95]
    some, some_blocks = SV.sense_extremes(model, token_ids=rows, count=6, _debug_blocks=True)
    tv, ti, bv, bi = R.row_extremes(torch.cat(some_blocks), 6)
    assert (some.top_ids.cpu().numpy() == ti.reshape(3, K, 6)).all() and (some.bottom_ids.cpu().numpy() == bi.reshape(3, K, 6)).all()
    given = SV.sense_extremes(model, contents=model.transformer.sense_table()[rows], count=6)
    assert torch.equal(given.top_ids, some.top_ids) and torch.equal(given.bottom_logits, some.bottom_logits)


def test_a_whole_vocabulary_call_allocates_the_block_and_the_outputs():
    from src.utils import sense_vocab as SV
    _bp()
    model = _model(torch.bfloat16, vocab=50257, n_layer=1)
    vocab_rows = model.lm_head.weight.shape[0]
    assert vocab_rows == 50264
    rows, count, chunk = vocab_rows * K, 20, 8192
    model.transformer.sense_table()                                   # built (and kept by the model) before the measurement
    target = torch.zeros(vocab_rows, device=DEV)
    target[[11, 500, 40000]] = 1.0
    SV.sense_extremes(model, token_ids=[0, 1], count=count)            # BLAS workspaces, code objects
    SV.non_contextual_localize(target, model, last_token_id=2)
    block = chunk * vocab_rows * 2
    mib = 1 << 20

    def peak_of(fn):
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        out = fn()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base, out

    # sense_extremes: the block, and the outputs -- fp32 logits and int64 ids, (V k, count) at each end
    peak, res = peak_of(lambda: SV.sense_extremes(model, count=count, chunk_rows=chunk))
    outputs = rows * count * (4 + 8) * 2
    print(f'sense_extremes: peak {peak / mib:.1f} MiB, block {block / mib:.1f} MiB, outputs {outputs / mib:.1f} MiB')
    assert res.top_ids.shape == (vocab_rows, K, count)
    assert peak <= block + outputs + mib
    # non_contextual_localize: the block, the scores, the two per-row fp32 vectors (maximum and numerator) and two fp32
    # copies of a chunk of (chunk, d) operand rows
    peak, scores = peak_of(lambda: SV.non_contextual_localize(target, model, chunk_rows=chunk))
    figure = block + rows * 4 + 2 * rows * 4 + 2 * chunk * D * 4
    print(f'non_contextual_localize: peak {peak / mib:.1f} MiB, computed {figure / mib:.1f} MiB')
    assert scores.shape == (vocab_rows, K) and (scores[50256:] == 0).all() and torch.isfinite(scores[:50256]).all()
    assert peak <= figure + mib
