"""GPU: the inference-only forms of the fused add + LayerNorm (bp_add_layer_norm_chain, csrc/add_layer_norm.hip) and the
chained trunk forward built on them (GPTModel._forward_chained, Block._forward_chained).

Everything here is bit for bit (torch.equal): the forms only remove passes over memory, every sum keeps its order.

  second branch input   (x0a + x1) + x0b against two launches of the plain kernel, the first storing x0a + x1 in fp32
  embedding source      against word[ids] + pos[pos_ids] (torch's 16-bit add) followed by the plain launch
  ownership             outputs sit between sentinel rows; x1 keeps its bits unless it is the output; a refused call writes
                        nothing
  whole model           logits with the chained path on and off, in one process; KV-cached generation (which does not chain)

rows = 5 / 21: a partial workgroup of four rows.  cols = 384, 640, 768: two and three chunks per lane, the last one partly
filled at 384 and 640.  The inputs differ in magnitude (x1 ~ 8, x0a ~ 1, x0b ~ 1/64), so that another order of the two
additions changes bits -- `test_the_inputs_tell_the_order_of_the_additions` checks that on the CPU."""
import ctypes

import pytest
import torch

import bp_hip

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
F32 = torch.float32
DTYPES = [torch.bfloat16, torch.float16]
DTYPE_IDS = ['bf16', 'fp16']
EPS = 1e-5
ROWS = 5


def _inputs(rows, cols, dtype, w_f32, seed=0):
    g = torch.Generator().manual_seed(seed + cols)
    x0a = torch.randn(rows, cols, generator=g).to(dtype)
    x0b = (torch.randn(rows, cols, generator=g) / 64).to(dtype)
    x1 = torch.randn(rows, cols, generator=g) * 8
    wdt = F32 if w_f32 else dtype
    w = (1 + 0.1 * torch.randn(cols, generator=g)).to(wdt)
    b = (0.1 * torch.randn(cols, generator=g)).to(wdt)
    return [t.to(DEV) for t in (x0a, x0b, x1, w, b)]


def _plain(x0, x1, w, b, residual=True):
    """Today's launch: z = LN(x0 + x1), residual x0 + x1 in fp32."""
    return bp_hip.add_layer_norm(x0, x1, w, b, EPS, residual_dtype=F32, return_residual=residual)


def test_the_inputs_tell_the_order_of_the_additions():
    x0a, x0b, x1, _, _ = [t.cpu() for t in _inputs(ROWS, 768, torch.bfloat16, True)]
    want = (x0a.float() + x1) + x0b.float()
    assert not torch.equal(want, (x0b.float() + x1) + x0a.float())
    assert not torch.equal(want, (x0a.float() + x0b.float()) + x1)


@pytest.mark.parametrize('mode', ['x_out', 'z_only', 'in_place', 'no_x1'])
@pytest.mark.parametrize('w_f32', [False, True], ids=['w16', 'w32'])
@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize('cols', [384, 640, 768])
def test_second_branch_input_matches_two_launches(cols, dtype, w_f32, mode):
    x0a, x0b, x1, w, b = _inputs(ROWS, cols, dtype, w_f32)
    if mode == 'no_x1':
        x1 = None
    _, first = _plain(x0a, x1, w, b)                 # stores x0a + x1 exactly in fp32
    z_want, x_want = _plain(x0b, first, w, b)        # adds its branch output to it
    x1_before = None if x1 is None else x1.clone()
    if mode == 'z_only':
        z = bp_hip.add_layer_norm(x0a, x1, w, b, EPS, x0b=x0b, return_residual=False)
        assert torch.equal(z, z_want)
    elif mode == 'in_place':
        z, x = bp_hip.add_layer_norm(x0a, x1, w, b, EPS, x0b=x0b, out_residual=x1)
        assert x is x1
        assert torch.equal(z, z_want) and torch.equal(x, x_want)
    else:
        z, x = bp_hip.add_layer_norm(x0a, x1, w, b, EPS, x0b=x0b)
        assert x.dtype == F32 and torch.equal(z, z_want) and torch.equal(x, x_want)
    assert z.dtype == dtype
    if mode in ('x_out', 'z_only'):
        assert torch.equal(x1, x1_before)


@pytest.mark.parametrize('w_f32', [False, True], ids=['w16', 'w32'])
@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize('cols', [384, 640, 768])
def test_inference_kernel_alone_matches_the_plain_launch(cols, dtype, w_f32):
    """No second input: norm2 of the chain (z alone), and the same with the residual, fresh and in place."""
    x0a, _, x1, w, b = _inputs(ROWS, cols, dtype, w_f32)
    z_want, x_want = _plain(x0a, x1, w, b)
    assert torch.equal(bp_hip.add_layer_norm(x0a, x1, w, b, EPS, return_residual=False, inference=True), z_want)
    z, x = bp_hip.add_layer_norm(x0a, x1, w, b, EPS, inference=True)
    assert torch.equal(z, z_want) and torch.equal(x, x_want)
    z, x = bp_hip.add_layer_norm(x0a, x1, w, b, EPS, out_residual=x1)
    assert x is x1 and torch.equal(z, z_want) and torch.equal(x, x_want)
    z_want, x_want = _plain(x0a, None, w, b)
    z, x = bp_hip.add_layer_norm(x0a, None, w, b, EPS, inference=True)
    assert torch.equal(z, z_want) and torch.equal(x, x_want)


def _tables(cols, dtype, vocab=53, npos=16, seed=3):
    g = torch.Generator().manual_seed(seed + cols)
    word = torch.randn(vocab, cols, generator=g).to(dtype).to(DEV)
    pos = torch.randn(npos, cols, generator=g).to(dtype).to(DEV)
    ids = torch.randint(0, vocab, (3, 7), generator=g)
    ids[0, 0], ids[0, 1], ids[1, 3], ids[2, 6], ids[2, 5] = 0, vocab - 1, vocab - 1, 0, int(ids[2, 4])   # ends and repeats
    return word, pos, ids.to(DEV)


@pytest.mark.parametrize('positions', ['none_given', 'shared_row', 'per_row', 'no_table'])
@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize('cols', [384, 640, 768])
def test_embedding_source_matches_gather_add_and_launch(cols, dtype, positions):
    word, pos, ids = _tables(cols, dtype)
    _, x0b, _, w, b = _inputs(ids.numel(), cols, dtype, True)
    x0b = x0b.view(*ids.shape, cols)
    pos_ids = None
    if positions == 'shared_row':
        pos_ids = torch.tensor([3, 0, 15, 15, 7, 1, 2], device=DEV)
    elif positions == 'per_row':
        pos_ids = torch.randint(0, 16, ids.shape, generator=torch.Generator().manual_seed(5)).to(DEV)
        pos_ids[0, 0], pos_ids[2, 6] = 15, 0
    if positions == 'no_table':                     # the content module's ln_0: words alone
        emb, source = word[ids], (ids, None, word, None)
    else:
        at = pos_ids if pos_ids is not None else torch.arange(ids.shape[1], device=DEV)
        emb, source = word[ids] + pos[at], (ids, pos_ids, word, pos)
    assert emb.dtype == dtype
    z_want, x_want = _plain(emb, None, w, b)
    assert torch.equal(x_want, emb.float())
    z = bp_hip.add_layer_norm(None, None, w, b, EPS, embedding=source, return_residual=False)       # ln_0
    assert z.shape == emb.shape and torch.equal(z, z_want)
    z, x = bp_hip.add_layer_norm(None, None, w, b, EPS, embedding=source)
    assert torch.equal(z, z_want) and torch.equal(x, x_want)
    z2_want, x2_want = _plain(x0b, x_want, w, b)                                                    # first block's norm1
    z2, x2 = bp_hip.add_layer_norm(None, None, w, b, EPS, embedding=source, x0b=x0b)
    assert torch.equal(z2, z2_want) and torch.equal(x2, x2_want)


def test_ids_outside_the_tables_read_their_last_row():
    word, pos, ids = _tables(384, torch.bfloat16)
    _, _, _, w, b = _inputs(ids.numel(), 384, torch.bfloat16, True)
    wild = ids.clone()
    wild[1, 1], wild[1, 2] = word.shape[0] + 5, -1          # (as unsigned values: both beyond the table)
    ids[1, 1] = ids[1, 2] = word.shape[0] - 1
    want = bp_hip.add_layer_norm(None, None, w, b, EPS, embedding=(ids, None, word, pos))
    got = bp_hip.add_layer_norm(None, None, w, b, EPS, embedding=(wild, None, word, pos))
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


# ---- ownership: through the C ABI, every output a window of a sentinel-filled buffer ---------------------------------------

def _chain(x0a, x0b, x1, tok, pos_ids, word, pos, w, b, z, xo, rows, cols, table_rows, pos_rows, pos_len, dtype):
    ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None   # noqa: E731
    rc = bp_hip.lib().bp_add_layer_norm_chain(
        ptr(x0a), ptr(x0b), ptr(x1), ptr(tok), ptr(pos_ids), ptr(word), ptr(pos), ptr(w), ptr(b), ptr(z), ptr(xo), rows, cols,
        table_rows, pos_rows, pos_len, EPS, 1 if dtype == torch.bfloat16 else 0, int(w.dtype == F32),
        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc


def _framed(rows, cols, dtype, guard=2):
    """(buffer of rows + 2 * guard rows filled with a sentinel, its window of `rows` rows)"""
    buf = torch.full((rows + 2 * guard, cols), -77.0, dtype=dtype, device=DEV)
    return buf, buf[guard:guard + rows]


def _guards_intact(buf, rows, guard=2):
    return bool((buf[:guard] == -77.0).all()) and bool((buf[guard + rows:] == -77.0).all())


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize('cols', [384, 640, 768])
def test_outputs_stay_inside_their_rows(cols, dtype):
    x0a, x0b, x1, w, b = _inputs(ROWS, cols, dtype, True)
    z_want, x_want = bp_hip.add_layer_norm(x0a, x1, w, b, EPS, x0b=x0b)
    zbuf, z = _framed(ROWS, cols, dtype)
    xbuf, xo = _framed(ROWS, cols, F32)
    x1_before = x1.clone()
    assert _chain(x0a, x0b, x1, None, None, None, None, w, b, z, xo, ROWS, cols, 0, 0, 0, dtype) == 0
    assert torch.equal(z, z_want) and torch.equal(xo, x_want)
    assert _guards_intact(zbuf, ROWS) and _guards_intact(xbuf, ROWS)
    assert torch.equal(x1, x1_before)
    # in place: the residual buffer is input and output, its guard rows stay
    xbuf[2:2 + ROWS] = x1
    zbuf[2:2 + ROWS] = -77.0
    assert _chain(x0a, x0b, xo, None, None, None, None, w, b, z, xo, ROWS, cols, 0, 0, 0, dtype) == 0
    assert torch.equal(z, z_want) and torch.equal(xo, x_want)
    assert _guards_intact(zbuf, ROWS) and _guards_intact(xbuf, ROWS)
    # embedding source, z alone: 21 rows
    word, pos, ids = _tables(cols, dtype)
    rows = ids.numel()
    want = bp_hip.add_layer_norm(None, None, w, b, EPS, embedding=(ids, None, word, pos), return_residual=False)
    zbuf, z = _framed(rows, cols, dtype)
    assert _chain(None, None, None, ids, None, word, pos, w, b, z, None, rows, cols, word.shape[0], pos.shape[0], ids.shape[1],
                  dtype) == 0
    assert torch.equal(z, want.view(rows, cols)) and _guards_intact(zbuf, rows)


def test_a_refused_call_writes_nothing():
    cols, dtype = 384, torch.bfloat16
    x0a, x0b, x1, w, b = _inputs(ROWS, cols, dtype, True)
    word, pos, ids = _tables(cols, dtype)
    rows = ids.numel()
    zbuf, z = _framed(rows, cols, dtype, guard=0)
    xbuf, xo = _framed(rows, cols, F32, guard=0)
    ok = dict(x0a=None, x0b=None, x1=None, tok=ids, pos_ids=None, word=word, pos=pos, w=w, b=b, z=z, xo=xo, rows=rows,
              cols=cols, table_rows=word.shape[0], pos_rows=pos.shape[0], pos_len=ids.shape[1], dtype=dtype)
    refused = [
        dict(x0a=x0a),                        # two sources of x0a
        dict(word=None, pos=None),            # none
        dict(tok=None),                       # tables without ids
        dict(pos=None, pos_ids=ids),          # position ids without a table
        dict(pos_len=4),                      # rows are no multiple of the positions' period
        dict(pos_len=0),
        dict(table_rows=0),
        dict(pos_rows=0),
        dict(cols=386),                       # cols % 4
        dict(cols=2052),                      # wider than the inference forms take
        dict(rows=0),
        dict(w=None),
        dict(z=None),
        dict(word=word.view(-1)[4:]),         # 8 bytes off a 16-byte boundary
        dict(tok=ids.view(torch.int32)[:, 1:]),   # ids 4 bytes off
    ]
    for change in refused:
        args = dict(ok, **change)
        if args['w'] is None:
            args['w'], w_null = b, True
        else:
            w_null = False
        if w_null:
            rc = bp_hip.lib().bp_add_layer_norm_chain(
                None, None, None, ids.data_ptr(), None, word.data_ptr(), pos.data_ptr(), None, b.data_ptr(), z.data_ptr(),
                xo.data_ptr(), rows, cols, word.shape[0], pos.shape[0], ids.shape[1], EPS, 1, 1, None)
            torch.cuda.synchronize()
        else:
            rc = _chain(**args)
        assert rc != 0, change
        assert bool((zbuf == -77.0).all()) and bool((xbuf == -77.0).all()), change
    assert bp_hip.lib().bp_add_layer_norm_chain(
        None, None, None, ids.data_ptr(), None, word.data_ptr(), pos.data_ptr(), w.data_ptr(), b.data_ptr(), z.data_ptr(),
        xo.data_ptr(), rows, cols, word.shape[0], pos.shape[0], ids.shape[1], EPS, 7, 1, None) == -1      # dtype
    assert bool((zbuf == -77.0).all()) and bool((xbuf == -77.0).all())
    assert _chain(**ok) == 0                  # (the unchanged arguments are accepted)
    # the binding refuses before it allocates or launches
    for kw in (dict(x0b=x0b[:, :380]), dict(x0b=x0b.float()), dict(x0b=x0b, dropout_p=0.1),
               dict(x0b=x0b, residual_dtype=dtype), dict(out_residual=x1.to(dtype)), dict(out_residual=x1[:4])):
        with pytest.raises(RuntimeError):
            bp_hip.add_layer_norm(x0a, x1, w, b, EPS, **kw)
    with pytest.raises(RuntimeError):
        bp_hip.add_layer_norm(x0a, None, w, b, EPS, embedding=(ids, None, word, pos))
    with pytest.raises(RuntimeError):
        bp_hip.add_layer_norm(None, None, w, b, EPS, embedding=(ids.int(), None, word, pos))


# ---- whole model ---------------------------------------------------------------------------------------------------------------

def _model(seq, **dims):
    from src.models.backpack import BackpackConfig, BackpackLMHeadModel
    torch.manual_seed(11)
    cfg = BackpackConfig(vocab_size=50257, n_positions=seq, scale_attn_by_inverse_layer_idx=True, resid_pdrop=0.0,
                         embd_pdrop=0.0, attn_pdrop=0.0, use_flash_attn=True, fused_bias_fc=True, fused_dense_gelu_dense=True,
                         fused_dropout_add_ln=True, pad_vocab_size_multiple=8, dedup_min_positions=1, **dims)
    return BackpackLMHeadModel(cfg, device=DEV, dtype=torch.bfloat16).eval()


class _Calls:
    """Names of the library's entry points as bp_hip calls them."""

    def __init__(self, monkeypatch):
        self.names = []
        inner = bp_hip._call

        def spy(name, *args):
            self.names.append(name)
            return inner(name, *args)

        monkeypatch.setattr(bp_hip, '_call', spy)

    def take(self):
        names, self.names = self.names, []
        return names


@pytest.mark.parametrize('name, dims, batch, seq', [
    ('micro', dict(n_embd=384, n_head=6, n_layer=6, num_content_vectors=16), 2, 128),
    ('small_2_layers', dict(n_embd=768, n_head=12, n_layer=2, num_content_vectors=16), 1, 1024),
], ids=['micro', 'small_2_layers'])
def test_whole_model_logits_do_not_change(monkeypatch, name, dims, batch, seq):
    model = _model(seq, **dims)
    trunk = model.transformer.gpt2_model
    calls = _Calls(monkeypatch)
    ids = torch.randint(0, 50257, (batch, seq), generator=torch.Generator().manual_seed(1)).to(DEV)
    n_layer = dims['n_layer']
    for order in ('batch', 'off'):              # the content network per distinct token / per position
        model.transformer.sense_table_mode = order
        with torch.no_grad():
            trunk.ln_chain = True
            calls.take()
            chained = model(ids).logits
            on = calls.take()
            trunk.ln_chain = False
            plain = model(ids).logits
            off = calls.take()
        trunk.ln_chain = True
        # ln_0, every norm1 and every norm2 are chain launches; what is left of the plain ones is the content network's
        assert on.count('bp_add_layer_norm_chain') == 1 + 2 * n_layer and 'bp_add_layer_norm_chain' not in off
        assert off.count('bp_dropout_add_layer_norm_scaled') - on.count('bp_dropout_add_layer_norm_scaled') == 1 + 2 * n_layer
        assert torch.equal(chained, plain), order
    # given position ids, shared and per sample
    with torch.no_grad():
        for pos in (torch.arange(seq, device=DEV).flip(0), torch.arange(seq, device=DEV).expand(batch, seq).contiguous()):
            trunk.ln_chain = True
            chained = model(ids, position_ids=pos).logits
            trunk.ln_chain = False
            assert torch.equal(chained, model(ids, position_ids=pos).logits)
    trunk.ln_chain = True
    # training, autograd and fp32 weights keep today's launches
    with torch.no_grad():
        model.train()
        calls.take()
        model(ids[:, :64])
        assert 'bp_add_layer_norm_chain' not in calls.take()
        model.eval()
    model(ids[:, :64])
    assert 'bp_add_layer_norm_chain' not in calls.take()


def test_kv_cached_generation_gives_the_same_tokens(monkeypatch):
    model = _model(128, n_embd=384, n_head=6, n_layer=6, num_content_vectors=16)
    trunk = model.transformer.gpt2_model
    calls = _Calls(monkeypatch)
    prompt = torch.randint(0, 50257, (2, 9), generator=torch.Generator().manual_seed(2)).to(DEV)
    trunk.ln_chain = True
    calls.take()
    on = model.generate(prompt, max_length=24, kv_cache=True)
    assert 'bp_add_layer_norm_chain' not in calls.take()          # cached steps go through Block.forward
    trunk.ln_chain = False
    off = model.generate(prompt, max_length=24, kv_cache=True)
    trunk.ln_chain = True
    assert torch.equal(on, off)
    # the growing-prefix loop runs whole forwards: it chains, and picks the same tokens
    whole_on = model.generate(prompt, max_length=16)
    assert 'bp_add_layer_norm_chain' in calls.take()
    trunk.ln_chain = False
    assert torch.equal(whole_on, model.generate(prompt, max_length=16))
    trunk.ln_chain = True
