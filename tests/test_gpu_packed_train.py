"""GPU: a training step on a PACKED batch (BackpackConfig.packed_train): every parameter gradient against the same model on the
right-padded batch through the fixed-length kernels, with the fp32 CPU eager model as truth and the whole-model rule of
test_gpu_backward.py (4 x the padded step's own error + 2 % of the gradient's scale)."""
import pytest
import torch

from flash_attn.losses.cross_entropy import CrossEntropyLoss
from src.models.backpack import BackpackConfig, BackpackLMHeadModel
from src.utils.packing import pack_sequences, packed_lm_labels

pytestmark = pytest.mark.gpu

DEV = 'cuda'
KW = dict(n_embd=64, n_head=2, n_layer=2, num_content_vectors=4, vocab_size=512, n_positions=160,
          scale_attn_by_inverse_layer_idx=True, resid_pdrop=0.0, embd_pdrop=0.0, attn_pdrop=0.0, pad_vocab_size_multiple=8)
HIP = dict(use_flash_attn=True, fused_dropout_add_ln=True, fused_bias_fc=True, fused_dense_gelu_dense=True)
LENGTHS = (160, 1, 37, 129)


def _models():
    torch.manual_seed(13)
    ref = BackpackLMHeadModel(BackpackConfig(use_flash_attn=False, **KW)).train()
    with torch.no_grad():
        ref.transformer.contextualization_attn.Wqkv.weight.mul_(6.0)
    hips = []
    for packed_train in (False, True):
        m = BackpackLMHeadModel(BackpackConfig(packed_train=packed_train, **HIP, **KW)).train()
        m.load_state_dict(ref.state_dict())
        hips.append(m.to(DEV, torch.bfloat16))
    return ref, hips[0], hips[1]


def test_packed_training_step_against_the_padded_one():
    ref, padded_model, packed_model = _models()
    ids = torch.randint(1, 512, (len(LENGTHS), max(LENGTHS)), generator=torch.Generator().manual_seed(5))
    labels = torch.full_like(ids, -100)
    for b, n in enumerate(LENGTHS):
        ids[b, n:] = 0
        labels[b, :n - 1] = ids[b, 1:n]
    packed, cu, longest = pack_sequences(ids, list(LENGTHS), device=DEV)

    logits = ref(ids).logits
    torch.nn.functional.cross_entropy(logits.reshape(-1, logits.shape[-1]), labels.reshape(-1), ignore_index=-100).backward()
    logits = padded_model(ids.to(DEV)).logits
    l_padded = CrossEntropyLoss()(logits.reshape(-1, logits.shape[-1]), labels.to(DEV).reshape(-1))
    l_padded.backward()
    logits = packed_model(packed, cu_seqlens=cu, max_seqlen=longest).logits
    assert logits.shape[0] == sum(LENGTHS)
    l_packed = CrossEntropyLoss()(logits, packed_lm_labels(packed, cu))
    l_packed.backward()

    assert abs(l_packed.item() - l_padded.item()) <= 2e-2
    for (name, p_ref), p_pad, p_pack in zip(ref.named_parameters(), padded_model.parameters(), packed_model.parameters()):
        assert p_pack.grad is not None, name
        r = p_ref.grad
        err = (p_pack.grad.float().cpu() - r).abs().max().item()
        base = (p_pad.grad.float().cpu() - r).abs().max().item()
        scale = max(r.abs().max().item(), 1e-6)
        print(f'packed train {name}: packed {err:.3e} padded {base:.3e} scale {scale:.3e}')
        assert err <= 4 * base + 2e-2 * scale, (name, err, base, scale)


def test_the_default_config_still_refuses_a_packed_batch_with_gradients():
    _, padded_model, _ = _models()
    packed, cu, longest = pack_sequences([[1, 2, 3], [4, 5]], device=DEV)
    with pytest.raises(RuntimeError, match='inference-only'):
        padded_model(packed, cu_seqlens=cu, max_seqlen=longest)
