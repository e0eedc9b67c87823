"""ctypes binding of libbackpack_hip.so (C ABI: include/bp_hip.h).

This is the only place where Python touches the native library.  torch is used for what the
reference's pybind layer used ATen for: device memory, the current stream and output allocation
(csrc/flash_attn/fmha_api.cpp:211,267-276).  There is NO fallback: if the shared library is
missing or a call fails, a RuntimeError is raised (the reference raises ImportError /
RuntimeError in the same situations, flash_attn/flash_attn_interface.py:5).
"""
import contextlib
import ctypes
import math
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('BP_HIP_LIB') or os.path.join(_HERE, 'libbackpack_hip.so')  # env: A/B builds only
ABI_VERSION = 11

_lib = None

# Backward routes that are NOT the fused HIP kernels -- autograd through an eager recomputation of the attention for head
# dims the HIP backward lacks (flash_attn_interface._FlashAttnFuncBase._bwd), the alpha-rebuilding backward of the sense
# mix for key-weighted / non-multiple-of-8 shapes (_sense_mix_backward_rebuild), the eager LayerNorm backward for rows wider
# than 2048 columns (flash_attn/ops/layer_norm.py) -- are opt-in: without
# `with bp_hip.allow_eager_fallback():` they raise instead of running silently (round-3 review: "no fallback" must mean it).
_eager_fallback = False


@contextlib.contextmanager
def allow_eager_fallback(enabled=True):
    """Within the block, backward passes whose shape the fused HIP kernels do not take may use the slower routes named
    above (they need (B, k, S, S)-sized buffers / eager attention).  Wrapping EITHER the forward or the backward() call is
    enough: the autograd Functions record the flag in their context at forward time (`fallback_recorded`) and also read it
    when backward runs.  The flag itself is process-wide on purpose: autograd runs the backward of CUDA tensors on its own
    device thread, where a thread-local set by the caller of backward() would not be seen."""
    global _eager_fallback
    previous, _eager_fallback = _eager_fallback, bool(enabled)
    try:
        yield
    finally:
        _eager_fallback = previous


def eager_fallback_allowed(ctx=None):
    """The flag now, or what `ctx` (an autograd context) recorded when its forward ran."""
    return bool(_eager_fallback or getattr(ctx, 'fallback_recorded', False))


_i32, _i64, _f32, _ptr = ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_void_p

# name -> (restype, argtypes); must list every symbol include/bp_hip.h declares
SIGNATURES = {
    'bp_strerror': (ctypes.c_char_p, [_i32]),
    'bp_abi_version': (_i32, []),
    'bp_build_flags': (_i32, []),
    'bp_flash_fwd': (_i32, [_ptr] * 7 + [_i32] * 5 + [_i64] * 9 + [_f32, _i32, _i32, _ptr]),
    'bp_flash_fwd_dropout': (_i32, [_ptr] * 7 + [_i32] * 5 + [_i64] * 9 + [_f32, _i32, _i32, _f32, _ptr, _ptr]),
    'bp_flash_bwd_ws_floats': (_i64, [_i32, _i32, _i64]),
    'bp_flash_bwd': (_i32, [_ptr] * 7 + [_i64] + [_ptr] * 5 + [_i32] * 5 + [_i64] * 17 + [_f32, _i32, _i32, _ptr]),
    'bp_flash_bwd_dropout': (_i32, [_ptr] * 7 + [_i64] + [_ptr] * 5 + [_i32] * 5 + [_i64] * 17
                             + [_f32, _i32, _i32, _f32, _ptr, _ptr]),
    'bp_attn_probs': (_i32, [_ptr] * 4 + [_i32] * 5 + [_i64] * 10 + [_f32, _i32, _i32, _ptr]),
    'bp_attn_probs_dropout': (_i32, [_ptr] * 4 + [_i32] * 5 + [_i64] * 10 + [_f32, _i32, _i32, _f32, _ptr, _ptr]),
    'bp_sense_lse': (_i32, [_ptr] * 2 + [_i32] * 4 + [_i64] * 4 + [_f32, _i32, _ptr]),
    'bp_sense_alpha': (_i32, [_ptr] * 3 + [_i32] * 5 + [_i64] * 4 + [_f32, _i32, _ptr]),
    'bp_sense_mix': (_i32, [_ptr] * 4 + [_i32] * 6 + [_i64] * 9 + [_f32, _i32, _ptr, _ptr]),
    'bp_sense_mix_weighted': (_i32, [_ptr] * 5 + [_i32] * 6 + [_i64] * 11 + [_f32, _i32, _ptr, _ptr]),
    'bp_sense_mix_gather': (_i32, [_ptr] * 5 + [_i32] * 6 + [_i64] * 10 + [_f32, _i32, _ptr, _ptr]),
    'bp_sense_lse_varlen': (_i32, [_ptr] * 3 + [_i32] * 4 + [_i64] * 3 + [_f32, _i32, _ptr]),
    'bp_sense_mix_varlen': (_i32, [_ptr] * 4 + [_i32, _ptr] + [_i32] * 5 + [_i64] * 6 + [_f32, _i32, _ptr, _ptr]),
    'bp_sense_mix_gather_varlen': (_i32, [_ptr] * 5 + [_i32, _ptr] + [_i32] * 5 + [_i64] * 7 + [_f32, _i32, _ptr, _ptr]),
    'bp_sense_mix_dc': (_i32, [_ptr] * 4 + [_i32] * 5 + [_i64] * 9 + [_f32, _i32, _ptr, _ptr]),
    'bp_sense_dq_dk': (_i32, [_ptr] * 6 + [_i32] * 5 + [_i64] * 11 + [_f32, _i32, _ptr]),
    'bp_add_layer_norm': (_i32, [_ptr] * 6 + [_i64, _i32, _f32] + [_i32] * 4 + [_ptr]),
    'bp_dropout_add_layer_norm': (_i32, [_ptr] * 7 + [_i64, _i32, _f32] + [_i32] * 5 + [_f32, _ptr, _ptr]),
    'bp_dropout_add_layer_norm_bwd': (_i32, [_ptr] * 9 + [_i64, _i32, _f32] + [_i32] * 4 + [_f32, _ptr, _ptr]),
    'bp_ln_bwd_ws_floats': (_i64, [_i32, _i32]),
    'bp_dropout_add_layer_norm_scaled': (_i32, [_ptr] * 9 + [_i64, _i32, _f32] + [_i32] * 5 + [_f32, _ptr, _ptr]),
    'bp_dropout_add_layer_norm_scaled_bwd': (_i32, [_ptr] * 13 + [_i64, _i64, _i32, _f32] + [_i32] * 4 + [_f32, _ptr, _ptr]),
    'bp_add_layer_norm_chain': (_i32, [_ptr] * 11 + [_i64, _i32] + [_i64] * 3 + [_f32, _i32, _i32, _ptr]),
    'bp_softmax_bwd_causal': (_i32, [_ptr, _ptr, _i64, _i32, _f32, _i32, _ptr]),
    'bp_add_layer_norm_bwd': (_i32, [_ptr] * 9 + [_i64, _i32, _f32, _i32, _i32, _i32, _ptr]),
    'bp_xentropy_fwd': (_i32, [_ptr] * 4 + [_i64, _i32, _i64, _f32, _i32, _i32, _ptr]),
    'bp_xentropy_bwd': (_i32, [_ptr] * 5 + [_i64, _i32, _i64, _i64, _f32, _i32, _i32, _ptr]),
    'bp_bias_grad_ws_floats': (_i64, [_i64, _i32]),
    'bp_bias_gelu_fwd': (_i32, [_ptr] * 4 + [_i64, _i32, _i32, _ptr]),
    'bp_bias_gelu_bwd': (_i32, [_ptr] * 5 + [_i64, _i32, _i32, _i32, _ptr]),
    'bp_column_sum': (_i32, [_ptr] * 3 + [_i64, _i32, _i32, _i32, _ptr]),
    'bp_flash_decode_ws_floats': (_i64, [_i32] * 4),
    'bp_flash_decode': (_i32, [_ptr] * 8 + [_i64] + [_i32] * 4 + [_i64] * 13 + [_f32, _i32, _ptr]),
    'bp_sense_decode_ws_floats': (_i64, [_i32] * 4),
    'bp_sense_decode': (_i32, [_ptr] * 9 + [_i64] + [_i32] * 5 + [_i64] + [_i64] * 11 + [_f32, _i32, _ptr]),
    'bp_sense_decode_weighted': (_i32, [_ptr] * 10 + [_i64] + [_i32] * 5 + [_i64] + [_i64] * 13 + [_f32, _i32, _ptr]),
    'bp_sense_rows_dot': (_i32, [_ptr] * 6 + [_i32] * 4 + [_i64] + [_i64] * 6 + [_i32, _ptr]),
    'bp_pick_token': (_i32, [_ptr] * 6 + [_i32] * 2 + [_i64] * 3 + [_i32] * 2 + [_f32, _i32, _f32, _i32, _ptr]),
    'bp_pick_token_ctl': (_i32, [_ptr] * 7 + [_i32] * 2 + [_i64] * 3 + [_i32] * 2 + [_f32, _i32, _f32, _f32] + [_i32] * 4 + [_ptr]),
    'bp_pick_token_lim': (_i32, [_ptr] * 7 + [_i32] * 2 + [_i64] * 3 + [_i32] * 2 + [_f32, _i32, _f32, _f32] + [_i32] * 3
                          + [_i32, _f32, _f32, _i32, _ptr, _i32, _i32, _ptr]),
    'bp_pick_token_lim_rows': (_i32, [_ptr] * 7 + [_i32] * 2 + [_i64] * 3 + [_i32] * 2 + [_f32, _i32, _f32, _f32] + [_i32] * 3
                               + [_i32, _f32, _f32, _i32, _ptr, _i32, _ptr, _ptr, _i32, _ptr]),
    'bp_pick_token_phrases': (_i32, [_ptr] * 7 + [_i32] * 2 + [_i64] * 3 + [_i32] * 2 + [_f32, _i32, _f32, _f32] + [_i32] * 3
                              + [_i32, _f32, _f32, _i32, _ptr, _i32, _ptr, _ptr] + [_ptr, _ptr, _i32, _i32] * 2
                              + [_ptr, _ptr, _i32, _ptr]),
    'bp_beam_pick_ws_floats': (_i64, [_i32] * 2),
    'bp_beam_pick': (_i32, [_ptr] * 8 + [_i64] + [_i32] * 3 + [_i64] * 3 + [_i32] * 4 + [_ptr]),
    'bp_beam_copy_rows': (_i32, [_ptr] * 3 + [_i32] + [_ptr] * 2 + [_i32] * 3 + [_ptr]),
    'bp_scatter_packed_rows': (_i32, [_ptr] * 6 + [_i32, _ptr, _i32, _i64, _i32, _i32, _ptr]),
    'bp_segment_sum_rows': (_i32, [_ptr] * 4 + [_i64, _i64, _i32, _i64, _i64, _i32, _i32, _ptr]),
    'bp_row_extremes': (_i32, [_ptr] * 5 + [_i32] * 2 + [_i64] + [_i32] * 2 + [_ptr]),
    'bp_sense_attribute_ws_floats': (_i64, [_i32] * 2),
    'bp_sense_attribute': (_i32, [_ptr] * 9 + [_i64] + [_i32] * 7 + [_i64] + [_i64] * 14 + [_f32, _i32, _ptr]),
    'bp_sense_similarity': (_i32, [_ptr] * 9 + [_i64] + [_i32] * 3 + [_i64] + [_i64] * 7 + [_i32, _ptr]),
    'bp_score_rows': (_i32, [_ptr] * 7 + [_i64, _i32, _i32] + [_i64] * 3 + [_i32, _ptr]),
    'bp_pick_report': (_i32, [_ptr] * 8 + [_i32] * 2 + [_i64] * 2 + [_i32, _i64, _i32, _i32, _ptr]),
    'bp_gemm_bf16': (_i32, [_ptr] * 4 + [_i64, _i32, _i32] + [_i64] * 3 + [_i32, _ptr, _i32, _ptr, _ptr]),
    'bp_gemm_f16': (_i32, [_ptr] * 4 + [_i64, _i32, _i32] + [_i64] * 3 + [_i32, _ptr, _i32, _ptr, _ptr]),
    'bp_gemm_library': (_i32, [_ptr, _ptr, _i32]),
    'bp_gemm_heuristic': (_i32, [_i32, _i32, _i64, _i32, _i32] + [_i64] * 3 + [_ptr, _i32, _ptr]),
}


def lib():
    """Load (once) and return the native library; raise loudly if it is not there."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f'{LIB_PATH} is missing: build it with `python backpacks-flash-attn_amd/build_hip.py` '
                '(or __graft_entry__.build()).  There is no non-HIP fallback for this path.')
        handle = ctypes.CDLL(LIB_PATH)
        for name, (restype, argtypes) in SIGNATURES.items():
            fn = getattr(handle, name)
            fn.restype = restype
            fn.argtypes = argtypes
        if handle.bp_abi_version() != ABI_VERSION:
            raise RuntimeError('libbackpack_hip.so ABI version mismatch; rebuild it')
        flags = handle.bp_build_flags()
        if flags & 3:
            # timing builds (-DBP_FWD_WHATIF / -DBP_BWD_WHATIF) delete work on purpose: never as the default library
            if not os.environ.get('BP_HIP_LIB'):
                raise RuntimeError(f'{LIB_PATH} is a what-if TIMING build (bp_build_flags() = {flags}): its results are '
                                   'garbage; rebuild without -DBP_FWD_WHATIF / -DBP_BWD_WHATIF')
            import warnings
            warnings.warn(f'bp_hip: {LIB_PATH} is a what-if timing build (flags {flags}): results are garbage on purpose')
        _lib = handle
    return _lib


def is_available():
    return os.path.exists(LIB_PATH)


def _check(code, what):
    if code != 0:
        raise RuntimeError(f'{what} failed: {lib().bp_strerror(code).decode()} (code {code})')


def _dtype_code(t):
    if t.dtype == torch.float16:
        return 0
    if t.dtype == torch.bfloat16:
        return 1
    raise RuntimeError(f'bp_hip: expected fp16 or bf16 tensors, got {t.dtype}')


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _call(name, device, *args):
    """Entry point `name` of the library on `device`: the current stream is read inside the device context (that
    device's stream) and appended to `args`; a failure code raises."""
    with torch.cuda.device(device):
        code = getattr(lib(), name)(*args, _stream())
    _check(code, name)


def _require_cuda(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError('bp_hip: tensors must live on the GPU (no CPU fallback exists)')


def round_up(x, m):
    return (x + m - 1) // m * m


def new_rng_state(device, generator=None):
    """Two fresh int64 words {seed, offset} ON THE DEVICE, drawn from torch's CUDA generator (so
    `torch.manual_seed` makes dropout reproducible) or from the caller's `generator` -- the role of the
    at::Generator philox state the reference hands its kernels (csrc/flash_attn/fmha_api.cpp:314-320, `gen_`
    argument).  Staying on the device keeps the call free of host synchronisation and legal inside HIP-graph
    capture; save the tensor to regenerate the mask in backward.  A CPU generator is accepted too (its two words
    are copied to the device: one small host-to-device transfer)."""
    if generator is not None and torch.device(generator.device).type != torch.device(device).type:
        return torch.randint(-2 ** 63, 2 ** 63 - 1, (2,), dtype=torch.int64, generator=generator).to(device)
    return torch.randint(-2 ** 63, 2 ** 63 - 1, (2,), dtype=torch.int64, device=device, generator=generator)


def _dropout_args(dropout_p, rng_state, device):
    dropout_p = float(dropout_p)
    if not 0.0 <= dropout_p < 1.0:
        raise RuntimeError('bp_hip: dropout_p must be in [0, 1)')
    if dropout_p == 0.0:
        return 0.0, None, None
    if rng_state is None:
        rng_state = new_rng_state(device)
    if rng_state.dtype != torch.int64 or rng_state.numel() != 2 or not rng_state.is_cuda \
            or not rng_state.is_contiguous():
        raise RuntimeError('bp_hip: rng_state must be a contiguous int64 tensor of 2 elements on the GPU')
    return dropout_p, rng_state, rng_state.data_ptr()


def flash_fwd(q, k, v, out, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, softmax_scale,
              causal, dropout_p=0.0, rng_state=None):
    """q (total_q,H,D), k/v (total_k,H,D), out like q (written in place); returns
    softmax_lse (B,H,roundup(max_seqlen_q,16)) fp32.  cu_seqlens_* int32 (B+1) or both None for a
    fixed-length batch whose size is total_q // max_seqlen_q.
    dropout_p > 0: attention dropout inside the kernel from `rng_state` (new_rng_state; created when None --
    pass your own to be able to hand the same state to flash_bwd / attn_probs)."""
    dropout_p, rng_state, rng_ptr = _dropout_args(dropout_p, rng_state, q.device)
    _require_cuda(q, k, v, out, cu_seqlens_q, cu_seqlens_k)
    if q.dim() != 3 or k.dim() != 3:
        raise RuntimeError('bp_hip.flash_fwd: q, k, v must be (total, nheads, headdim)')
    if not (q.dtype == k.dtype and (v is None or (v.dtype == q.dtype and out.dtype == q.dtype))):
        raise RuntimeError('bp_hip.flash_fwd: q, k, v, out must share one dtype')
    for t in (q, k, v, out):
        if t is not None and t.stride(-1) != 1:
            raise RuntimeError('bp_hip.flash_fwd: last dimension must be contiguous')
    total_q, nheads, d = q.shape
    if k.shape[1] != nheads or k.shape[2] != d or (v is not None and v.shape != k.shape):
        raise RuntimeError('bp_hip.flash_fwd: q/k/v shape mismatch')
    if v is not None and out.shape != q.shape:
        raise RuntimeError('bp_hip.flash_fwd: out must have the shape of q')
    if cu_seqlens_q is not None:
        for cu in (cu_seqlens_q, cu_seqlens_k):
            if cu.dtype != torch.int32 or not cu.is_contiguous():
                raise RuntimeError('bp_hip.flash_fwd: cu_seqlens must be contiguous int32')
        batch = cu_seqlens_q.numel() - 1
        if cu_seqlens_k.numel() - 1 != batch:
            raise RuntimeError('bp_hip.flash_fwd: cu_seqlens_q / cu_seqlens_k length mismatch')
    else:
        batch = total_q // max_seqlen_q
        if batch * max_seqlen_q != total_q or batch * max_seqlen_k != k.shape[0]:
            raise RuntimeError('bp_hip.flash_fwd: fixed-length batch does not divide total rows')
    if batch <= 0:
        raise RuntimeError('bp_hip.flash_fwd: empty batch')
    # (Callers that KNOW the batch is fixed-length pass cu_seqlens = None -- the modules of this package do; the row
    # count alone does not say so: an over-allocated (B * max_seqlen)-row buffer with shorter sequences in cu_seqlens is
    # legal, as in the reference's mha_fwd, which only reads the offsets.)
    lse_len = round_up(max_seqlen_q, 16)
    lse = torch.empty((batch, nheads, lse_len), dtype=torch.float32, device=q.device)
    _call('bp_flash_fwd_dropout', q.device,
          q.data_ptr(), k.data_ptr(), v.data_ptr() if v is not None else None,
          out.data_ptr() if out is not None else None, lse.data_ptr(),
          cu_seqlens_q.data_ptr() if cu_seqlens_q is not None else None,
          cu_seqlens_k.data_ptr() if cu_seqlens_k is not None else None,
          batch, nheads, d, int(max_seqlen_q), int(max_seqlen_k),
          q.stride(0), q.stride(1), k.stride(0), k.stride(1),
          v.stride(0) if v is not None else 0, v.stride(1) if v is not None else 0,
          out.stride(0) if out is not None else 0, out.stride(1) if out is not None else 0,
          lse_len, float(softmax_scale), int(bool(causal)), _dtype_code(q), dropout_p, rng_ptr)
    return lse


def flash_bwd_supported(q):
    """Shapes the HIP backward covers (others recompute eagerly in the autograd Functions)."""
    return (q.is_cuda and q.dtype in (torch.float16, torch.bfloat16) and q.shape[-1] % 8 == 0
            and q.shape[-1] <= 128)


def flash_bwd(dout, q, k, v, out, softmax_lse, dq, dk, dv, cu_seqlens_q, cu_seqlens_k, max_seqlen_q,
              max_seqlen_k, softmax_scale, causal, dropout_p=0.0, rng_state=None):
    """dq, dk, dv (written in place) of the fused attention; arguments as the reference's
    _flash_attn_backward (flash_attn/flash_attn_interface.py:31-47).  `out` and `softmax_lse` are
    the forward's results; with dropout, (dropout_p, rng_state) must be the forward's."""
    if float(dropout_p) > 0.0 and rng_state is None:
        raise RuntimeError('bp_hip.flash_bwd: dropout_p > 0 needs the rng_state the forward used')
    dropout_p, rng_state, rng_ptr = _dropout_args(dropout_p, rng_state, q.device)
    _require_cuda(dout, q, k, v, out, softmax_lse, dq, dk, dv, cu_seqlens_q, cu_seqlens_k)
    # the same checks as flash_fwd, plus the gradient buffers: a mismatched dk/dv or a wrong max_seqlen would
    # otherwise be an out-of-bounds write inside the kernel (the reference checks these in mha_bwd,
    # csrc/flash_attn/fmha_api.cpp:375-420)
    if q.dim() != 3 or k.dim() != 3:
        raise RuntimeError('bp_hip.flash_bwd: q, k, v must be (total, nheads, headdim)')
    total_q, nheads, d = q.shape
    for name, t, like in (('k', k, None), ('v', v, k), ('out', out, q), ('dout', dout, q), ('dq', dq, q),
                          ('dk', dk, k), ('dv', dv, k)):
        if t.dtype != q.dtype:
            raise RuntimeError(f'bp_hip.flash_bwd: {name} must have the dtype of q')
        if like is not None and t.shape != like.shape:
            raise RuntimeError(f'bp_hip.flash_bwd: {name} has shape {tuple(t.shape)}, expected {tuple(like.shape)}')
    if k.shape[1] != nheads or k.shape[2] != d:
        raise RuntimeError('bp_hip.flash_bwd: q/k shape mismatch')
    for name, t in (('q', q), ('k', k), ('v', v), ('dq', dq), ('dk', dk), ('dv', dv)):
        if t.stride(-1) != 1:
            raise RuntimeError(f'bp_hip.flash_bwd: last dimension of {name} must be contiguous')
    if dout.stride(-1) != 1:
        dout = dout.contiguous()
    if cu_seqlens_q is not None:
        if cu_seqlens_k is None:
            raise RuntimeError('bp_hip.flash_bwd: cu_seqlens_q and cu_seqlens_k must be given together')
        for cu in (cu_seqlens_q, cu_seqlens_k):
            if cu.dtype != torch.int32 or not cu.is_contiguous():
                raise RuntimeError('bp_hip.flash_bwd: cu_seqlens must be contiguous int32')
        batch = cu_seqlens_q.numel() - 1
        if cu_seqlens_k.numel() - 1 != batch:
            raise RuntimeError('bp_hip.flash_bwd: cu_seqlens_q / cu_seqlens_k length mismatch')
    else:
        if cu_seqlens_k is not None:
            raise RuntimeError('bp_hip.flash_bwd: cu_seqlens_q and cu_seqlens_k must be given together')
        batch = total_q // max_seqlen_q
        if batch * max_seqlen_q != total_q or batch * max_seqlen_k != k.shape[0]:
            raise RuntimeError('bp_hip.flash_bwd: fixed-length batch does not divide total rows')
    if batch <= 0:
        raise RuntimeError('bp_hip.flash_bwd: empty batch')
    if softmax_lse.dtype != torch.float32 or not softmax_lse.is_contiguous() or \
            softmax_lse.shape != (batch, nheads, round_up(max_seqlen_q, 16)):
        raise RuntimeError('bp_hip.flash_bwd: softmax_lse must be the contiguous fp32 (batch, nheads, '
                           'roundup(max_seqlen_q, 16)) tensor the forward returned')
    lse_len = softmax_lse.shape[-1]
    if out.stride(-1) != 1:
        out = out.contiguous()
    # workspace for the row statistics -D_i = -sum_d dO_i[d] * O_i[d] and -L_i / scale (filled by the dQ kernel, read
    # by the dK/dV kernel)
    dsum = torch.empty(int(lib().bp_flash_bwd_ws_floats(batch, nheads, lse_len)), dtype=torch.float32, device=q.device)
    _call('bp_flash_bwd_dropout', q.device,
          dout.data_ptr(), q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(),
          softmax_lse.data_ptr(), dsum.data_ptr(), dsum.numel(), dq.data_ptr(), dk.data_ptr(), dv.data_ptr(),
          cu_seqlens_q.data_ptr() if cu_seqlens_q is not None else None,
          cu_seqlens_k.data_ptr() if cu_seqlens_k is not None else None,
          batch, nheads, d, int(max_seqlen_q), int(max_seqlen_k),
          dout.stride(0), dout.stride(1), q.stride(0), q.stride(1), k.stride(0), k.stride(1),
          v.stride(0), v.stride(1), out.stride(0), out.stride(1), dq.stride(0), dq.stride(1),
          dk.stride(0), dk.stride(1), dv.stride(0), dv.stride(1), lse_len, float(softmax_scale),
          int(bool(causal)), _dtype_code(q), dropout_p, rng_ptr)
    return dq, dk, dv


def attn_probs(q, k, lse, softmax_scale, causal, dropout_p=0.0, rng_state=None):
    """q (B,Sq,H,D), k (B,Sk,H,D) (any batch/row/head strides), lse (B,H,>=Sq) fp32 ->
    probabilities (B,H,Sq,Sk) in q's dtype.  With (dropout_p, rng_state) of a flash_fwd call: entries that
    call dropped carry a set SIGN BIT (decode with torch.signbit; kept / dropped magnitudes are the undropped P)."""
    _require_cuda(q, k, lse)
    if float(dropout_p) > 0.0 and rng_state is None:
        raise RuntimeError('bp_hip.attn_probs: dropout_p > 0 needs the rng_state of the forward call')
    dropout_p, rng_state, rng_ptr = _dropout_args(dropout_p, rng_state, q.device)
    b, sq, h, d = q.shape
    sk = k.shape[1]
    if q.stride(-1) != 1 or k.stride(-1) != 1 or not lse.is_contiguous():
        raise RuntimeError('bp_hip.attn_probs: bad strides')
    probs = torch.empty((b, h, sq, sk), dtype=q.dtype, device=q.device)
    _call('bp_attn_probs_dropout', q.device,
          q.data_ptr(), k.data_ptr(), lse.data_ptr(), probs.data_ptr(), b, h, d, sq, sk,
          q.stride(0), q.stride(1), q.stride(2), k.stride(0), k.stride(1), k.stride(2),
          lse.shape[-1], probs.stride(0), probs.stride(1), probs.stride(2),
          float(softmax_scale), int(bool(causal)), _dtype_code(q), dropout_p, rng_ptr)
    return probs


def _queue_ws(device):
    """The 64-byte ticket record of ONE persistent sense-mix launch (include/bp_hip.h: queue_ws).  A fresh tensor per
    call from torch's stream-ordered caching allocator: while a HIP graph is being captured it comes from the graph's
    private pool, so the graph owns the record it replays and no eager launch can ever share it.  The caller keeps the
    tensor in a local until the launch call has returned: the block then goes back to the allocator of the stream the
    launch was enqueued on (allocation and launch both use torch's CURRENT stream), whose reuse is stream-ordered."""
    return torch.empty(16, dtype=torch.int32, device=device)


def _check_qk(qk):
    _require_cuda(qk)
    if qk.dim() != 5 or qk.shape[2] != 2 or qk.stride(-1) != 1:
        raise RuntimeError('bp_hip: qk must be (B, S, 2, k, d_k) with a contiguous last dim')
    return qk.shape[0], qk.shape[1], qk.shape[3], qk.shape[4]


def _vec16(*tensors):
    """16-byte friendly layouts: 16-byte aligned bases, a unit last stride and every other stride a multiple of 8."""
    return all(t.data_ptr() % 16 == 0 and t.stride(-1) == 1 and all(s % 8 == 0 for s in t.stride()[:-1])
               for t in tensors)


def _sense_qk(qk, softmax_scale):
    """The preamble of the sense wrappers: (qk', b, s, k, d_k', scale), the scale defaulting to the TRUE d_k's.  The
    LDS-DMA kernels move 16-byte chunks, i.e. need d_k % 8 == 0.  The Mini k=64 ablation has d_k = 10
    (training/configs/experiment/owt/backpack-mini-flash-vecs-64.yaml): qk' zero-pads the head dimension to the next
    multiple of 8, d_k' (zeros add nothing to q.k), instead of falling to the element-wise loader."""
    b, s, k, dk = _check_qk(qk)
    scale = softmax_scale or dk ** -0.5
    if dk % 8:
        qk = torch.nn.functional.pad(qk, (0, (-dk) % 8))
    return qk, b, s, k, qk.shape[-1], scale


def sense_lse(qk, softmax_scale=None):
    """qk (B,S,2,k,d_k) -> lse (B,k,roundup(S,16)) fp32: log-sum-exp of every causal row."""
    qk, b, s, k, dk, scale = _sense_qk(qk, softmax_scale)
    lse = torch.empty((b, k, round_up(s, 16)), dtype=torch.float32, device=qk.device)
    _call('bp_sense_lse', qk.device, qk.data_ptr(), lse.data_ptr(), b, s, k, dk,
          qk.stride(0), qk.stride(1), qk.stride(2), qk.stride(3), float(scale), _dtype_code(qk))
    return lse


def _lse_ws(qk, lse, b, s, k):
    if lse is None:
        return torch.empty((b, k, round_up(s, 16)), dtype=torch.float32, device=qk.device), 0
    if lse.shape != (b, k, round_up(s, 16)) or lse.dtype != torch.float32 or not lse.is_contiguous():
        raise RuntimeError('bp_hip: lse must be the tensor returned by sense_lse for this qk')
    return lse, 1


def sense_alpha(qk, softmax_scale=None, lse=None):
    """qk (B,S,2,k,d_k) -> alpha (B,k,S,S), causal softmax over keys, exact zeros above the
    diagonal (replaces backpack.py:116-122).  `lse`: optional result of sense_lse(qk)."""
    qk, b, s, k, dk, scale = _sense_qk(qk, softmax_scale)
    alpha = torch.empty((b, k, s, s), dtype=qk.dtype, device=qk.device)
    ws, ready = _lse_ws(qk, lse, b, s, k)
    _call('bp_sense_alpha', qk.device, qk.data_ptr(), alpha.data_ptr(), ws.data_ptr(), ready, b, s, k, dk,
          qk.stride(0), qk.stride(1), qk.stride(2), qk.stride(3), float(scale), _dtype_code(qk))
    return alpha


def sense_mix(qk, content, softmax_scale=None, out=None, lse=None, key_weight=None):
    """Fused sum_l softmax_causal(q_l k_l^T * scale) @ C_l without materialising alpha.

    qk (B,S,2,k,d_k); content in its storage layout (B,S,k,d_out) (the reference's
    `content` (B,k,S,d_out) is `.transpose(1,2)` of it -- pass that view transposed back, it is
    free); returns (B,S,d_out).  Replaces backpack.py:305+313.
    key_weight (B,k,S), optional: alpha[b,l,:,s] (= content row s of sense l) is scaled by
    key_weight[b,l,s] inside the kernel -- the intervention hook of intervened_models.py:97-101 and
    test_genderbias.py:71-78 (C ABI bp_sense_mix_weighted)."""
    qk, b, s, k, dk, scale = _sense_qk(qk, softmax_scale)
    _require_cuda(content)
    if content.dim() != 4 or content.shape[:3] != (b, s, k) or content.stride(-1) != 1:
        raise RuntimeError('bp_hip.sense_mix: content must be (B, S, k, d_out), last dim contiguous')
    if content.dtype != qk.dtype:
        raise RuntimeError('bp_hip.sense_mix: qk and content dtypes differ')
    dout = content.shape[3]
    if out is None:
        out = torch.empty((b, s, dout), dtype=qk.dtype, device=qk.device)
    ws, ready = _lse_ws(qk, lse, b, s, k)
    kw = None
    if key_weight is not None:
        _require_cuda(key_weight)
        if key_weight.shape != (b, k, s):
            raise RuntimeError('bp_hip.sense_mix: key_weight must be (B, k, S)')
        kw = key_weight.to(torch.float32)
        if kw.stride(-1) != 1:
            kw = kw.contiguous()
    queue_ws = _queue_ws(qk.device)   # alive until the launch call has returned (stream-ordered reuse afterwards)
    _call('bp_sense_mix_weighted', qk.device,
          qk.data_ptr(), content.data_ptr(), kw.data_ptr() if kw is not None else None, out.data_ptr(),
          ws.data_ptr(), ready, b, s, k, dk, dout,
          qk.stride(0), qk.stride(1), qk.stride(2), qk.stride(3),
          content.stride(0), content.stride(1), content.stride(2),
          kw.stride(0) if kw is not None else 0, kw.stride(1) if kw is not None else 0,
          out.stride(0), out.stride(1), float(scale), _dtype_code(qk), queue_ws.data_ptr())
    return out


SENSE_MAX_DK = 640     # widest sense bp_sense_lse / _alpha / _mix take (include/bp_hip.h; > 128: csrc/sense_wide.hip)


WIDE_RING_DK = (160, 640)   # sense widths beyond 128 the LDS-DMA ring kernels take (csrc/sense_wide_dma.hip), with S % 32 == 0


def _gather_limits(qk, table, seqlen):
    """(exceeded, reason) of every limit of bp_sense_mix_gather (include/bp_hip.h): the 16-byte vector path, seqlen <= 4096,
    32-bit byte offsets into the table; senses up to 128 wide with at most 65 536 table rows (any GPT-2 vocabulary), or the
    reference's two few-sense widths (WIDE_RING_DK, seqlen a multiple of 32: the ring kernels of csrc/sense_wide_dma.hip,
    any row count)."""
    dk = round_up(qk.shape[-1], 8)
    wide = dk > 128
    rows = table.shape[0]
    return (
        (wide and not (dk in WIDE_RING_DK and seqlen % 32 == 0),
         f'sense width {qk.shape[-1]} > 128 and not {WIDE_RING_DK} at a sequence length that is a multiple of 32 '
         '(those senses take the dense kernel)'),
        (seqlen > 4096, f'sequence length {seqlen} > 4096 (a job keeps its keys\' row indices in LDS)'),
        (not wide and rows > 65536, f'{rows} table rows > 65536 (u16 row indices)'),
        (rows * table.stride(0) * table.element_size() >= 2 ** 32, 'table of 4 GiB or more (32-bit byte offsets)'),
        (not (qk.is_cuda and table.is_cuda), 'qk or table not on the GPU'),
        (table.dim() != 3 or table.shape[2] % 8 != 0 or not _vec16(table),
         'table layout (last dim contiguous, 16-byte aligned rows, d % 8 == 0 required)'),
        (wide and not _vec16(qk), 'qk layout (senses wider than 128 need 16-byte aligned rows)'),
    )


def sense_mix_gather_supported(qk, table, seqlen):
    """Shapes bp_sense_mix_gather takes: those that exceed none of its limits (_gather_limits)."""
    return not any(exceeded for exceeded, _ in _gather_limits(qk, table, seqlen))


def sense_mix_gather_limits(qk, table, seqlen):
    """Which limits of bp_sense_mix_gather a call exceeds, as text (callers log it when they fall back to a torch gather)."""
    return '; '.join(reason for exceeded, reason in _gather_limits(qk, table, seqlen) if exceeded)


def sense_mix_gather(qk, table, row_index, softmax_scale=None, out=None, lse=None):
    """sense_mix with the content rows read from a table: content[b, s, l, :] = table[row_index[b, s], l, :].

    qk (B,S,2,k,d_k); table (rows, k, d_out), e.g. the content network's output for the distinct tokens of the batch;
    row_index (B,S) int32 (torch.unique's inverse); returns (B,S,d_out).  The (B,S,k,d_out) content tensor of
    backpack.py:276 is never materialised (C ABI bp_sense_mix_gather)."""
    qk, b, s, k, dk, scale = _sense_qk(qk, softmax_scale)
    _require_cuda(table, row_index)
    if table.dim() != 3 or table.shape[1] != k or table.stride(-1) != 1:
        raise RuntimeError('bp_hip.sense_mix_gather: table must be (rows, k, d_out), last dim contiguous')
    if table.dtype != qk.dtype:
        raise RuntimeError('bp_hip.sense_mix_gather: qk and table dtypes differ')
    if row_index.shape != (b, s) or row_index.dtype != torch.int32 or row_index.stride(-1) != 1:
        raise RuntimeError('bp_hip.sense_mix_gather: row_index must be (B, S) int32, unit stride along S')
    dout = table.shape[2]
    if out is None:
        out = torch.empty((b, s, dout), dtype=qk.dtype, device=qk.device)
    ws, ready = _lse_ws(qk, lse, b, s, k)
    queue_ws = _queue_ws(qk.device)   # alive until the launch call has returned
    _call('bp_sense_mix_gather', qk.device,
          qk.data_ptr(), table.data_ptr(), row_index.data_ptr(), out.data_ptr(), ws.data_ptr(), ready,
          b, s, k, dk, dout, table.shape[0],
          qk.stride(0), qk.stride(1), qk.stride(2), qk.stride(3),
          table.stride(0), table.stride(1), row_index.stride(0),
          out.stride(0), out.stride(1), float(scale), _dtype_code(qk), queue_ws.data_ptr())
    return out


# ---- packed batches (C ABI bp_sense_*_varlen): sample b owns rows [cu_seqlens[b], cu_seqlens[b + 1]) -----------------------

def _check_packed_qk(qk, cu_seqlens, max_seqlen, who):
    _require_cuda(qk, cu_seqlens)
    if qk.dim() != 4 or qk.shape[1] != 2 or qk.stride(-1) != 1:
        raise RuntimeError(f'bp_hip.{who}: qk must be (total, 2, k, d_k) with a contiguous last dim')
    if cu_seqlens.dim() != 1 or cu_seqlens.numel() < 2 or cu_seqlens.dtype != torch.int32 or not cu_seqlens.is_contiguous():
        raise RuntimeError(f'bp_hip.{who}: cu_seqlens must be a contiguous (batch + 1,) int32 tensor')
    if int(max_seqlen) < 1:
        raise RuntimeError(f'bp_hip.{who}: max_seqlen must be >= 1')
    return qk.shape[0], cu_seqlens.numel() - 1, qk.shape[2], qk.shape[3]


def _varlen_limits(qk, values, max_seqlen, gather):
    """(exceeded, reason) of every limit of bp_sense_mix_varlen / bp_sense_mix_gather_varlen (include/bp_hip.h): narrow senses
    on the 16-byte vector path; the gathering form (`values` = the table) additionally bp_sense_mix_gather's own limits."""
    rows = values.shape[0]
    return (
        (qk.shape[-1] > 128, f'sense width {qk.shape[-1]} > 128 (no packed wide kernels)'),
        (qk.shape[-1] % 8 != 0, f'sense width {qk.shape[-1]} not a multiple of 8'),
        (not (qk.is_cuda and values.is_cuda), 'qk or content not on the GPU'),
        (qk.dtype not in (torch.float16, torch.bfloat16), f'dtype {qk.dtype} (fp16 / bf16 only)'),
        (not _vec16(qk), 'qk layout (16-byte aligned rows required)'),
        (values.dim() != 3 or values.shape[2] % 8 != 0 or not _vec16(values),
         'content / table layout (last dim contiguous, 16-byte aligned rows, d % 8 == 0 required)'),
        (max_seqlen > 65536, f'max_seqlen {max_seqlen} > 65536'),
        (gather and max_seqlen > 4096, f'max_seqlen {max_seqlen} > 4096 (a job keeps its keys\' row indices in LDS)'),
        (gather and rows > 65536, f'{rows} table rows > 65536 (u16 row indices)'),
        (gather and rows * values.stride(0) * values.element_size() >= 2 ** 32, 'table of 4 GiB or more (32-bit byte offsets)'),
    )


def sense_mix_varlen_supported(qk, content, max_seqlen):
    """Shapes bp_sense_mix_varlen takes (qk (total, 2, k, d_k), content (total, k, d_out))."""
    return not any(exceeded for exceeded, _ in _varlen_limits(qk, content, max_seqlen, False))


def sense_mix_varlen_limits(qk, content, max_seqlen):
    """Which limits of bp_sense_mix_varlen a call exceeds, as text (callers name it when they pad the batch instead)."""
    return '; '.join(reason for exceeded, reason in _varlen_limits(qk, content, max_seqlen, False) if exceeded)


def sense_mix_gather_varlen_supported(qk, table, max_seqlen):
    """Shapes bp_sense_mix_gather_varlen takes (qk (total, 2, k, d_k), table (rows, k, d_out))."""
    return not any(exceeded for exceeded, _ in _varlen_limits(qk, table, max_seqlen, True))


def sense_mix_gather_varlen_limits(qk, table, max_seqlen):
    """Which limits of bp_sense_mix_gather_varlen a call exceeds, as text."""
    return '; '.join(reason for exceeded, reason in _varlen_limits(qk, table, max_seqlen, True) if exceeded)


def sense_lse_varlen(qk, cu_seqlens, max_seqlen, softmax_scale=None):
    """qk (total,2,k,d_k), cu_seqlens (B+1,) int32 -> lse (B,k,roundup(max_seqlen,16)) fp32: log-sum-exp of every causal row
    of every sequence of the packed batch; entries at or behind a sequence's length are not written.  cu_seqlens is not
    validated (include/bp_hip.h); src/utils/packing.py builds checked ones."""
    total, b, k, dk = _check_packed_qk(qk, cu_seqlens, max_seqlen, 'sense_lse_varlen')
    scale = softmax_scale or dk ** -0.5
    lse = torch.empty((b, k, round_up(int(max_seqlen), 16)), dtype=torch.float32, device=qk.device)
    _call('bp_sense_lse_varlen', qk.device, qk.data_ptr(), lse.data_ptr(), cu_seqlens.data_ptr(), b, int(max_seqlen), k, dk,
          qk.stride(0), qk.stride(1), qk.stride(2), float(scale), _dtype_code(qk))
    return lse


def _packed_out_lse(who, qk, total, b, k, max_seqlen, dout, out, lse):
    if out is None:
        out = torch.empty((total, dout), dtype=qk.dtype, device=qk.device)
    elif out.shape != (total, dout) or out.dtype != qk.dtype or out.stride(-1) != 1 or not out.is_cuda:
        raise RuntimeError(f'bp_hip.{who}: out must be (total, d_out) in qk\'s dtype on the GPU, last dim contiguous')
    ws, ready = _lse_ws(qk, lse, b, int(max_seqlen), k)
    return out, ws, ready


def sense_mix_varlen(qk, content, cu_seqlens, max_seqlen, softmax_scale=None, out=None, lse=None):
    """sense_mix on a packed batch: qk (total,2,k,d_k), content (total,k,d_out), cu_seqlens (B+1,) int32 -> (total,d_out).
    Every sequence attends causally within its own rows; its output rows carry the bits of sense_mix on that sequence
    alone.  `lse`: optional result of sense_lse_varlen.  Narrow senses on the 16-byte path only
    (sense_mix_varlen_supported; C ABI bp_sense_mix_varlen)."""
    total, b, k, dk = _check_packed_qk(qk, cu_seqlens, max_seqlen, 'sense_mix_varlen')
    _require_cuda(content)
    if content.dim() != 3 or content.shape[:2] != (total, k) or content.stride(-1) != 1:
        raise RuntimeError('bp_hip.sense_mix_varlen: content must be (total, k, d_out), last dim contiguous')
    if content.dtype != qk.dtype:
        raise RuntimeError('bp_hip.sense_mix_varlen: qk and content dtypes differ')
    scale = softmax_scale or dk ** -0.5
    dout = content.shape[2]
    out, ws, ready = _packed_out_lse('sense_mix_varlen', qk, total, b, k, max_seqlen, dout, out, lse)
    queue_ws = _queue_ws(qk.device)   # alive until the launch call has returned
    _call('bp_sense_mix_varlen', qk.device,
          qk.data_ptr(), content.data_ptr(), out.data_ptr(), ws.data_ptr(), ready,
          cu_seqlens.data_ptr(), b, int(max_seqlen), k, dk, dout,
          qk.stride(0), qk.stride(1), qk.stride(2), content.stride(0), content.stride(1), out.stride(0),
          float(scale), _dtype_code(qk), queue_ws.data_ptr())
    return out


def sense_mix_gather_varlen(qk, table, row_index, cu_seqlens, max_seqlen, softmax_scale=None, out=None, lse=None):
    """sense_mix_gather on a packed batch: content[t, l, :] = table[row_index[t], l, :] for the packed row t.
    qk (total,2,k,d_k), table (rows,k,d_out), row_index (total,) int32 -> (total,d_out)
    (sense_mix_gather_varlen_supported; C ABI bp_sense_mix_gather_varlen)."""
    total, b, k, dk = _check_packed_qk(qk, cu_seqlens, max_seqlen, 'sense_mix_gather_varlen')
    _require_cuda(table, row_index)
    if table.dim() != 3 or table.shape[1] != k or table.stride(-1) != 1:
        raise RuntimeError('bp_hip.sense_mix_gather_varlen: table must be (rows, k, d_out), last dim contiguous')
    if table.dtype != qk.dtype:
        raise RuntimeError('bp_hip.sense_mix_gather_varlen: qk and table dtypes differ')
    if row_index.shape != (total,) or row_index.dtype != torch.int32 or row_index.stride(-1) != 1:
        raise RuntimeError('bp_hip.sense_mix_gather_varlen: row_index must be (total,) int32, unit stride')
    scale = softmax_scale or dk ** -0.5
    dout = table.shape[2]
    out, ws, ready = _packed_out_lse('sense_mix_gather_varlen', qk, total, b, k, max_seqlen, dout, out, lse)
    queue_ws = _queue_ws(qk.device)   # alive until the launch call has returned
    _call('bp_sense_mix_gather_varlen', qk.device,
          qk.data_ptr(), table.data_ptr(), row_index.data_ptr(), out.data_ptr(), ws.data_ptr(), ready,
          cu_seqlens.data_ptr(), b, int(max_seqlen), k, dk, dout, table.shape[0],
          qk.stride(0), qk.stride(1), qk.stride(2), table.stride(0), table.stride(1), out.stride(0),
          float(scale), _dtype_code(qk), queue_ws.data_ptr())
    return out


def _ln_16bit_code(*tensors):
    """dtype code of the 16-bit type in play (x0 / residual / weights may each be 16-bit or fp32)."""
    for t in tensors:
        if t is not None and t.dtype in (torch.float16, torch.bfloat16):
            return _dtype_code(t), t.dtype
    return 1, torch.bfloat16


def _ln_scales(x0, weight, rowscale, colscale):
    """Checked, contiguous (rowscale, colscale) of the fused LayerNorm: rowscale one value per row in x0's dtype,
    colscale one per column in the weights' dtype (reference: csrc/layer_norm/ln_api.cpp:122-135)."""
    cols = x0.shape[-1]
    if rowscale is not None:
        _require_cuda(rowscale)
        if rowscale.numel() != x0.numel() // cols or rowscale.dtype != x0.dtype:
            raise RuntimeError('bp_hip.add_layer_norm: rowscale must hold one value per row, in x0\'s dtype')
        rowscale = rowscale.contiguous()
    if colscale is not None:
        _require_cuda(colscale)
        if colscale.shape != (cols,) or colscale.dtype != weight.dtype:
            raise RuntimeError('bp_hip.add_layer_norm: colscale (layerscale) must be (cols,) in the weights\' dtype')
        colscale = colscale.contiguous()
    return rowscale, colscale


def _add_layer_norm_chain(x0, x1, weight, bias, eps, return_residual, x0b, embedding, out_residual):
    """The inference-only forms of add_layer_norm (bp_add_layer_norm_chain); everything is checked before the launch."""
    if embedding is not None:
        if x0 is not None:
            raise RuntimeError('bp_hip.add_layer_norm: give x0 or `embedding`, not both')
        token_ids, position_ids, word, pos_table = embedding
        _require_cuda(token_ids, position_ids, word, pos_table)
        if word.dim() != 2 or word.dtype not in (torch.float16, torch.bfloat16) or not word.is_contiguous():
            raise RuntimeError('bp_hip.add_layer_norm: the word table must be a contiguous 16-bit (rows, cols) matrix')
        if token_ids.dtype != torch.int64 or not token_ids.is_contiguous() or token_ids.numel() == 0:
            raise RuntimeError('bp_hip.add_layer_norm: token ids must be a contiguous, non-empty int64 tensor')
        if x1 is not None:
            raise RuntimeError('bp_hip.add_layer_norm: the embedding source takes no residual input (it is the stream so far)')
        dt16, cols, shape, pos_len = word.dtype, word.shape[1], tuple(token_ids.shape) + (word.shape[1],), 0
        if pos_table is not None:
            if pos_table.dim() != 2 or pos_table.shape[1] != cols or pos_table.dtype != dt16 or not pos_table.is_contiguous():
                raise RuntimeError('bp_hip.add_layer_norm: the position table must be a contiguous (rows, cols) matrix of '
                                   'the word table\'s dtype')
            pos_len = token_ids.shape[-1]
            if position_ids is not None:
                # what broadcasting against the ids allows here: one position per row, or one row of them shared by all
                if position_ids.dtype != torch.int64 or not position_ids.is_contiguous() or \
                        (tuple(position_ids.shape) != tuple(token_ids.shape) and position_ids.numel() != pos_len) or \
                        position_ids.shape[-1] != pos_len:
                    raise RuntimeError('bp_hip.add_layer_norm: position ids must be contiguous int64, shaped like the token '
                                       'ids or like their last dimension')
                pos_len = position_ids.numel()
        elif position_ids is not None:
            raise RuntimeError('bp_hip.add_layer_norm: position ids without a position table')
    else:
        _require_cuda(x0)
        if x0 is None or x0.dtype not in (torch.float16, torch.bfloat16):
            raise RuntimeError('bp_hip.add_layer_norm: the inference forms take a 16-bit x0')
        dt16, cols, shape = x0.dtype, x0.shape[-1], tuple(x0.shape)
        x0 = x0.contiguous()
    _require_cuda(x1, x0b, weight, bias, out_residual)
    if weight.shape != (cols,) or bias.shape != (cols,) or weight.dtype != bias.dtype or \
            weight.dtype not in (torch.float32, dt16):
        raise RuntimeError('bp_hip.add_layer_norm: weight/bias must be (cols,), both fp32 or both the 16-bit dtype in use')
    if cols > 2048:
        raise RuntimeError('bp_hip.add_layer_norm: the inference forms take rows of up to 2048 columns')
    if x0b is not None:
        if tuple(x0b.shape) != shape or x0b.dtype != dt16:
            raise RuntimeError('bp_hip.add_layer_norm: x0b must have the shape and the 16-bit dtype of x0')
        x0b = x0b.contiguous()
    if x1 is not None:
        if tuple(x1.shape) != shape or x1.dtype != torch.float32:
            raise RuntimeError('bp_hip.add_layer_norm: the inference forms take an fp32 residual of x0\'s shape')
        if out_residual is not x1:
            x1 = x1.contiguous()
    if out_residual is not None:
        if not return_residual:
            raise RuntimeError('bp_hip.add_layer_norm: out_residual without return_residual')
        if tuple(out_residual.shape) != shape or out_residual.dtype != torch.float32 or not out_residual.is_contiguous():
            raise RuntimeError('bp_hip.add_layer_norm: out_residual must be a contiguous fp32 tensor of x0\'s shape')
    device = weight.device
    z = torch.empty(shape, dtype=dt16, device=device)
    xo = None
    if return_residual:
        xo = out_residual if out_residual is not None else torch.empty(shape, dtype=torch.float32, device=device)
    wc, bc = weight.contiguous(), bias.contiguous()
    ptr = lambda t: t.data_ptr() if t is not None else None   # noqa: E731
    if embedding is not None:
        source = (ptr(token_ids), ptr(position_ids), ptr(word), ptr(pos_table))
        sizes = (word.shape[0], pos_table.shape[0] if pos_table is not None else 0, pos_len)
    else:
        source, sizes = (None, None, None, None), (0, 0, 0)
    _call('bp_add_layer_norm_chain', device, ptr(x0), ptr(x0b), ptr(x1), *source, wc.data_ptr(), bc.data_ptr(),
          z.data_ptr(), ptr(xo), z.numel() // cols, cols, *sizes, float(eps), _dtype_code(z),
          int(weight.dtype == torch.float32))
    return (z, xo) if return_residual else z


def add_layer_norm(x0, x1, weight, bias, eps, residual_dtype=None, return_residual=True, dropout_p=0.0,
                   rng_state=None, return_dropout_mask=False, rowscale=None, colscale=None, x0b=None, embedding=None,
                   out_residual=None, inference=False):
    """Fused z = LayerNorm(dropout(x0) / (1 - p) + x1) (fp32 math) and the updated residual stream
    x = dropout(x0) / (1 - p) + x1.

    x0 (..., cols) fp16 / bf16 / fp32 contiguous; x1 same shape (fp32 or x0's dtype) or None; weight/bias
    (cols,) fp32 or 16-bit.  Returns (z in x0's dtype, x in residual_dtype) -- or z alone -- and, when asked,
    the uint8 keep mask (all ones without dropout).  residual_dtype defaults to x1's dtype (reference rule,
    csrc/layer_norm/ln_api.cpp:99-102).  Replaces dropout_add_layer_norm (flash_attn/ops/layer_norm.py:207-217).
    dropout_p > 0 draws from `rng_state` (new_rng_state; pass your own to hand the same state to
    add_layer_norm_bwd).  rowscale (one value per row, x0's dtype) / colscale (cols, the weights' dtype): x0 is multiplied
    by rowscale[row] before and by colscale[col] after the dropout -- DropPath and LayerScale (`rowscale`, `layerscale` of
    the reference's dropout_add_layer_norm).

    Inference-only forms (no dropout, no scales, no mask; 16-bit x0, fp32 residual), taken when one of these is given:
    x0b          a second 16-bit branch output: x = (x0 + x1) + x0b, added in this order -- bit for bit what a launch
                 that stores x0 + x1 in fp32 and a second one that adds x0b to it compute
    embedding    (token_ids int64, position_ids int64 or None, word_table, position_table or None) with x0 = None:
                 x0 is word_table[token_ids] (+ position_table[positions], one 16-bit add), gathered inside the kernel;
                 without position_ids the position is the index along token_ids' last dimension
    out_residual an fp32 tensor the residual stream is written to instead of a fresh one; it may be x1 itself
    inference    True: the inference kernel also with none of the three (same bits; it has every load of a row in flight at
                 once, where the general kernel decides operand by operand at run time)"""
    if inference or x0b is not None or embedding is not None or out_residual is not None:
        if dropout_p != 0.0 or return_dropout_mask or rowscale is not None or colscale is not None or \
                residual_dtype not in (None, torch.float32):
            raise RuntimeError('bp_hip.add_layer_norm: x0b / embedding / out_residual / inference are inference-only forms: no dropout, '
                               'no mask, no scales, an fp32 residual stream')
        return _add_layer_norm_chain(x0, x1, weight, bias, eps, return_residual, x0b, embedding, out_residual)
    _require_cuda(x0, x1, weight, bias)
    if x0.dtype not in (torch.float16, torch.bfloat16, torch.float32):
        raise RuntimeError(f'bp_hip.add_layer_norm: x0 must be fp16, bf16 or fp32, got {x0.dtype}')
    cols = x0.shape[-1]
    if weight.shape != (cols,) or bias.shape != (cols,) or weight.dtype != bias.dtype:
        raise RuntimeError('bp_hip.add_layer_norm: weight/bias must be (cols,) of one dtype')
    code_dt, dt16 = _ln_16bit_code(x0, x1, weight)
    x0_f32 = x0.dtype == torch.float32
    if weight.dtype not in (torch.float32, dt16):
        raise RuntimeError('bp_hip.add_layer_norm: weight dtype must be fp32 or the 16-bit dtype in use')
    x0c = x0.contiguous()
    x1c = None
    if x1 is not None:
        if x1.shape != x0.shape or x1.dtype not in (torch.float32, x0.dtype):
            raise RuntimeError('bp_hip.add_layer_norm: residual must match x0 (fp32 or input dtype)')
        x1c = x1.contiguous()
    if residual_dtype is None:
        residual_dtype = x1.dtype if x1 is not None else x0.dtype
    if residual_dtype not in (torch.float32, x0.dtype):
        raise RuntimeError('bp_hip.add_layer_norm: residual dtype must be fp32 or the input dtype')
    dropout_p, rng_state, rng_ptr = _dropout_args(dropout_p, rng_state, x0.device)
    z = torch.empty_like(x0c)
    xo = torch.empty(x0c.shape, dtype=residual_dtype, device=x0.device) if return_residual else None
    dmask = None
    if return_dropout_mask:
        dmask = (torch.empty(x0c.shape, dtype=torch.uint8, device=x0.device) if dropout_p > 0.0
                 else torch.ones(x0c.shape, dtype=torch.uint8, device=x0.device))
    rows = x0c.numel() // cols
    wc, bc = weight.contiguous(), bias.contiguous()
    rowscale, colscale = _ln_scales(x0c, weight, rowscale, colscale)
    _call('bp_dropout_add_layer_norm_scaled', x0.device,
          x0c.data_ptr(), x1c.data_ptr() if x1c is not None else None, wc.data_ptr(), bc.data_ptr(),
          rowscale.data_ptr() if rowscale is not None else None,
          colscale.data_ptr() if colscale is not None else None,
          z.data_ptr(), xo.data_ptr() if xo is not None else None,
          dmask.data_ptr() if (dmask is not None and dropout_p > 0.0) else None, rows, cols, float(eps), code_dt,
          int(x0_f32), int(x1c is not None and x1c.dtype == torch.float32), int(residual_dtype == torch.float32),
          int(weight.dtype == torch.float32), dropout_p, rng_ptr)
    outs = (z, xo) if return_residual else (z,)
    if return_dropout_mask:
        outs = outs + (dmask,)
    return outs if len(outs) > 1 else outs[0]


def softmax_bwd_causal_supported(alpha):
    return alpha.is_cuda and alpha.dtype in (torch.float16, torch.bfloat16) and alpha.shape[-1] % 8 == 0 \
        and alpha.shape[-1] <= 4096


def softmax_bwd_causal_(alpha, dalpha, softmax_scale):
    """In place: dalpha (..., S, S) <- scale * alpha * (dalpha - rowsum(alpha * dalpha)) below/on the diagonal,
    0 above it.  alpha as returned by sense_alpha.  Returns dalpha (now the gradient of the raw scores q.k)."""
    _require_cuda(alpha, dalpha)
    if alpha.shape != dalpha.shape or alpha.dtype != dalpha.dtype or not alpha.is_contiguous() \
            or not dalpha.is_contiguous() or alpha.shape[-1] != alpha.shape[-2]:
        raise RuntimeError('bp_hip.softmax_bwd_causal_: alpha and dalpha must be equal-shaped contiguous (..., S, S)')
    s = alpha.shape[-1]
    _call('bp_softmax_bwd_causal', alpha.device, alpha.data_ptr(), dalpha.data_ptr(), alpha.numel() // (s * s), s,
          float(softmax_scale), _dtype_code(alpha))
    return dalpha


SLAB = 128   # queries per slab of the dq / dk backward (fixed by the kernels)


def sense_mix_dc(qk, dout, lse, softmax_scale, like, out=None):
    """dcontent (B,S,k,d_out) of sense_mix: bp_sense_mix_dc (alpha recomputed from the saved lse, never stored).
    `like`: the forward's content tensor (last dimension / dtype / device of the result); `out`: a contiguous
    (B,S,k,d_out) buffer to write instead of a fresh one."""
    b, s, k, dk = _check_qk(qk)
    if out is None:
        out = torch.empty((b, s, k, like.shape[-1]), dtype=like.dtype, device=like.device)
    elif out.shape != (b, s, k, like.shape[-1]) or out.dtype != like.dtype or not out.is_contiguous() or not out.is_cuda:
        raise RuntimeError('bp_hip.sense_mix_dc: out must be a contiguous (B, S, k, d_out) GPU tensor of the content\'s dtype')
    dcontent = out
    queue_ws = _queue_ws(qk.device)
    _call('bp_sense_mix_dc', qk.device,
          qk.data_ptr(), dout.data_ptr(), lse.data_ptr(), dcontent.data_ptr(), b, s, k, dk, like.shape[-1],
          qk.stride(0), qk.stride(1), qk.stride(2), qk.stride(3), dout.stride(0), dout.stride(1),
          dcontent.stride(0), dcontent.stride(1), dcontent.stride(2), float(softmax_scale), _dtype_code(qk),
          queue_ws.data_ptr())
    return dcontent


def sense_dqk(qk, content, dout, lse, softmax_scale, out=None):
    """dqk (like qk) of sense_mix.  The 768-deep product dP_l[t,s] = dout[t].C[s,l] is a plain GEMM and goes to the
    BLAS library, slab by slab (128 queries), TRANSPOSED into a (B, S*k, 128) buffer that is reused: the content's
    own storage (B, S*k, d) is its left operand as it stands, so nothing is copied or permuted.  bp_sense_dq_dk then
    turns each slab into dq rows and dk contributions (softmax backward + the two thin products) on the fly.
    `out`: a contiguous tensor like qk to write instead of a fresh one."""
    b, s, k, dk = _check_qk(qk)
    d = content.shape[-1]
    c_flat = content.reshape(b, s * k, d)                      # a view for the (B,S,k,d) storage layout
    if out is None:
        out = torch.empty_like(qk)
    elif out.shape != qk.shape or out.dtype != qk.dtype or not out.is_contiguous() or not out.is_cuda:
        raise RuntimeError('bp_hip.sense_dqk: out must be a contiguous GPU tensor of qk\'s shape and dtype')
    dqk = out
    dk_acc = torch.zeros((b, s, k, dk), dtype=torch.float32, device=qk.device)
    dsum = torch.empty((b, k, round_up(s, 16)), dtype=torch.float32, device=qk.device)
    buf = torch.empty(b * s * k * SLAB, dtype=qk.dtype, device=qk.device)
    code_dt = _dtype_code(qk)
    for t0 in range(0, s, SLAB):
        n = min(s, t0 + SLAB) * k
        rows = dout[:, t0:t0 + SLAB]
        if rows.shape[1] < SLAB:                               # last, partial slab: pad the queries with zeros
            rows = torch.nn.functional.pad(rows, (0, 0, 0, SLAB - rows.shape[1]))
        dpt = buf[:b * n * SLAB].view(b, n, SLAB)
        torch.bmm(c_flat[:, :n], rows.transpose(1, 2), out=dpt)
        _call('bp_sense_dq_dk', qk.device,
              qk.data_ptr(), dpt.data_ptr(), lse.data_ptr(), dsum.data_ptr(), dqk.data_ptr(), dk_acc.data_ptr(),
              b, s, k, dk, t0, qk.stride(0), qk.stride(1), qk.stride(2), qk.stride(3), dpt.stride(0),
              dqk.stride(0), dqk.stride(1), dqk.stride(3), dk_acc.stride(0), dk_acc.stride(1), dk_acc.stride(2),
              float(softmax_scale), code_dt)
    dqk[:, :, 1] = dk_acc
    return dqk


def _fused_mix_backward_ok(qk, content, key_weight):
    return (key_weight is None and qk.shape[-1] % 8 == 0 and qk.shape[-1] <= 128 and content.shape[-1] % 8 == 0
            and qk.is_contiguous()
            and content.stride(-1) == 1 and content.stride(2) == content.shape[-1]
            and content.stride(1) == content.shape[2] * content.shape[-1]
            and content.stride(0) == content.shape[1] * content.stride(1) and qk.shape[1] <= 65536)


class SenseMixFn(torch.autograd.Function):
    """Differentiable fused sense contraction.  Forward: LSE pre-pass + bp_sense_mix_weighted (alpha never stored).
    Backward (second half), alpha recomputed from the saved LSE inside the kernels:
        dC_l = alpha_l^T dout                                   bp_sense_mix_dc   (the forward kernel, roles swapped)
        dP_l = dout C_l^T   (slabs of 128 queries, BLAS)  ->  dS = alpha (dP - rowsum(alpha dP))
        dq_l = scale dS k_l,  dk_l = scale dS^T q_l             bp_sense_dq_dk
    Peak extra memory: one (B, S*k, 128) 16-bit slab; the reference's autograd keeps three (B,k,S,S) fp32 tensors
    alive from the forward on.  With an intervention `key_weight` (inference-time experiments) or shapes the fused
    kernels do not take, the older alpha-rebuilding formulation below runs instead."""

    @staticmethod
    def forward(ctx, qk, content, softmax_scale, key_weight):
        scale = softmax_scale or qk.shape[-1] ** -0.5
        lse = sense_lse(qk, scale)
        out = sense_mix(qk, content, scale, lse=lse, key_weight=key_weight)
        ctx.save_for_backward(qk, content, lse, key_weight)
        ctx.scale = scale
        ctx.fallback_recorded = eager_fallback_allowed()
        return out

    @staticmethod
    def backward(ctx, dout):
        qk, content, lse, key_weight = ctx.saved_tensors
        dout = dout.contiguous()
        if not _fused_mix_backward_ok(qk, content, key_weight):
            # wide senses (128 < d_k <= 640: csrc/sense_wide.hip) have no fused backward and need none: with few senses
            # alpha is small (k S^2 per sample), so the alpha-rebuilding route IS their backward -- no opt-in asked
            wide = key_weight is None and qk.shape[-1] > 128
            if not wide and not eager_fallback_allowed(ctx):
                raise RuntimeError(
                    'bp_hip.SenseMixFn.backward: the fused backward kernels take d_k % 8 == 0, d_out % 8 == 0, a contiguous '
                    '(B,S,k,d) content and no key_weight; this call would take the alpha-rebuilding route (two (B,k,S,S) '
                    'buffers + BLAS GEMMs).  Opt in with `with bp_hip.allow_eager_fallback():` around the forward or around backward().')
            return _sense_mix_backward_rebuild(ctx, qk, content, lse, key_weight, dout)
        dcontent = sense_mix_dc(qk, dout, lse, ctx.scale, content) if ctx.needs_input_grad[1] else None
        dqk = sense_dqk(qk, content, dout, lse, ctx.scale) if ctx.needs_input_grad[0] else None
        return dqk, dcontent, None, None


def _sense_mix_backward_rebuild(ctx, qk, content, lse, key_weight, dout):
    """alpha rebuilt once by bp_sense_alpha from the saved LSE (two (B,k,S,S) 16-bit buffers), batched GEMMs,
    bp_softmax_bwd_causal in place, two thin GEMMs: the round-1 formulation, kept for key_weight / odd shapes."""
    b, s, _, k, dk = qk.shape
    alpha = sense_alpha(qk, ctx.scale, lse=lse)                               # (B,k,S,S)
    weighted = alpha if key_weight is None else alpha * key_weight.unsqueeze(2).to(alpha.dtype)
    g = dout.unsqueeze(1)                                                      # (B,1,S,d)
    dcontent = None
    if ctx.needs_input_grad[1]:
        dcontent = torch.matmul(weighted.transpose(2, 3), g).transpose(1, 2)   # (B,S,k,d) view of (B,k,S,d)
    dqk = None
    if ctx.needs_input_grad[0]:
        dalpha = torch.matmul(g, content.permute(0, 2, 3, 1))                  # (B,k,S_t,S_s)
        if key_weight is not None:
            dalpha = dalpha * key_weight.unsqueeze(2).to(dalpha.dtype)
        dqk = _scores_backward(qk, alpha, dalpha.contiguous(), ctx.scale)
    return dqk, dcontent, None, None


def _scores_backward(qk, alpha, dalpha, scale):
    """dqk (B,S,2,k,dk) from alpha (B,k,S,S) and its gradient dalpha (contiguous, overwritten): the causal softmax
    backward (bp_softmax_bwd_causal in place, an fp32 torch expression for shapes it does not take), then dq = dS k and
    dk = dS^T q."""
    if softmax_bwd_causal_supported(alpha):
        ds = softmax_bwd_causal_(alpha, dalpha, scale)
    else:
        a32, d32 = alpha.float(), dalpha.float()
        ds = (scale * a32 * (d32 - (a32 * d32).sum(-1, keepdim=True))).to(alpha.dtype)
    q, kk = qk[:, :, 0].transpose(1, 2), qk[:, :, 1].transpose(1, 2)       # (B,k,S,dk)
    dq = torch.matmul(ds, kk)
    dkk = torch.matmul(ds.transpose(2, 3), q)
    return torch.stack([dq.transpose(1, 2), dkk.transpose(1, 2)], dim=2)


def sense_mix_autograd(qk, content, softmax_scale=None, key_weight=None):
    """sense_mix that records a backward when gradients are enabled (training), the plain kernel otherwise."""
    if torch.is_grad_enabled() and (qk.requires_grad or content.requires_grad):
        return SenseMixFn.apply(qk, content, softmax_scale, key_weight)
    return sense_mix(qk, content, softmax_scale, key_weight=key_weight)


# ---- the sense mix over a table of rows, with a backward (training with the content network once per distinct token) -------

SEGMENT_LONG_ROWS = 32      # segments of at least this many rows take the kernel's second route (csrc/bp_kernels.h kSegLongRows)
SEGMENT_ROW_LANES = 16      # ... where 16 lanes take rows r, r + 16, ... each (csrc/segment_sum_rows.hip kSegRowLanes)
SEGMENT_UNROLL = 8          # rows a thread loads ahead on either route (kSegUnroll)


def segment_sum_rows(rows, order, seg_begin, acc, accumulate=False):
    """acc[u] (= or +=, `accumulate`) the fp32 sum of rows[order[i]] over i in [seg_begin[u], seg_begin[u + 1]): C ABI
    bp_segment_sum_rows, deterministic (no atomics; the bits depend on the inputs only).
    rows (n_rows, cols) fp16 / bf16, unit last stride, cols and the row stride multiples of 8; order (n_rows,) int32: the row
    numbers grouped by segment, ascending inside a segment; seg_begin (n_segments + 1,) int32, non-decreasing; acc
    (n_segments, cols) fp32, unit last stride.  With accumulate=False an empty segment's row is zeroed, with True it is
    left as it is.  Returns acc."""
    _require_cuda(rows, order, seg_begin, acc)
    if rows.dim() != 2 or rows.stride(1) != 1 or rows.shape[0] < 1 or rows.shape[1] % 8 or rows.stride(0) % 8 \
            or rows.data_ptr() % 16:
        raise RuntimeError('bp_hip.segment_sum_rows: rows must be (n_rows >= 1, cols), last dim contiguous, 16-byte aligned, '
                           'cols and the row stride multiples of 8')
    n_rows, cols = rows.shape
    if order.shape != (n_rows,) or order.dtype != torch.int32 or not order.is_contiguous():
        raise RuntimeError('bp_hip.segment_sum_rows: order must be a contiguous (n_rows,) int32 tensor')
    if seg_begin.dim() != 1 or seg_begin.shape[0] < 1 or seg_begin.dtype != torch.int32 or not seg_begin.is_contiguous():
        raise RuntimeError('bp_hip.segment_sum_rows: seg_begin must be a contiguous (n_segments + 1,) int32 tensor')
    n_segments = seg_begin.shape[0] - 1
    if acc.shape != (n_segments, cols) or acc.dtype != torch.float32 or acc.stride(1) != 1 or acc.stride(0) % 4 \
            or acc.data_ptr() % 16 or acc.stride(0) < cols:
        raise RuntimeError('bp_hip.segment_sum_rows: acc must be (n_segments, cols) fp32, last dim contiguous, 16-byte '
                           'aligned, rows that do not overlap, a row stride that is a multiple of 4')
    if len({rows.device, order.device, seg_begin.device, acc.device}) != 1:
        raise RuntimeError('bp_hip.segment_sum_rows: all tensors must live on one device')
    if n_segments:
        _call('bp_segment_sum_rows', rows.device, rows.data_ptr(), order.data_ptr(), seg_begin.data_ptr(), acc.data_ptr(),
              n_rows, n_segments, cols, rows.stride(0), acc.stride(0), int(bool(accumulate)), _dtype_code(rows))
    return acc


def row_segments(row_index, n_segments):
    """(order, seg_begin) of bp_segment_sum_rows for `row_index` (any shape, integer, values in [0, n_segments)): the
    positions grouped by the row they read, ascending inside a group (one STABLE sort), and where every row's group begins
    in that list.  All on the device, no host value read."""
    flat = row_index.reshape(-1)
    ordered, order = torch.sort(flat, stable=True)
    bounds = torch.arange(n_segments + 1, dtype=ordered.dtype, device=flat.device)
    return order.to(torch.int32), torch.searchsorted(ordered, bounds, out_int32=True)


def _gather_train_limits(qk, table, seqlen):
    b, s, _, k, dk = qk.shape
    return _gather_limits(qk, table, seqlen) + (
        (dk % 8 != 0 or dk > 128, f'sense width {dk} not a multiple of 8 or > 128 (the fused backward kernels)'),
        (not qk.is_contiguous() or not table.is_contiguous(), 'qk or table not contiguous'),
        (s > 65536, f'sequence length {s} > 65536'),
    )


def sense_mix_gather_train_shape_limits(d_k, seqlen):
    """What the sense width (before it is widened to a multiple of 8) and the sequence length alone rule out, as text: a
    caller can tell before it builds the table."""
    return '; '.join(reason for exceeded, reason in (
        (round_up(d_k, 8) > 128, f'sense width {d_k} > 128 (the fused backward kernels)'),
        (seqlen > 4096, f'sequence length {seqlen} > 4096 (bp_sense_mix_gather keeps a job\'s row indices in LDS)'),
    ) if exceeded)


def sense_mix_gather_train_supported(qk, table, seqlen):
    """Shapes SenseMixGatherFn takes: those of bp_sense_mix_gather that the fused backward kernels (bp_sense_mix_dc,
    bp_sense_dq_dk: _fused_mix_backward_ok) take as well."""
    return not any(exceeded for exceeded, _ in _gather_train_limits(qk, table, seqlen))


def sense_mix_gather_train_limits(qk, table, seqlen):
    """Which of those limits a call exceeds, as text."""
    return '; '.join(reason for exceeded, reason in _gather_train_limits(qk, table, seqlen) if exceeded)


class SenseMixGatherFn(torch.autograd.Function):
    """SenseMixFn with the content rows read from a table: content[b, s] = table[row_index[b, s]] is never materialised
    for the whole batch, neither in the forward (bp_sense_mix_gather) nor as a gradient.  The backward runs over chunks of
    `chunk_samples` samples and reuses two chunk-sized buffers:
        dcontent_c = bp_sense_mix_dc(qk[c], dout[c], lse[c])                  (c, S, k, d)
        dtable    += bp_segment_sum_rows(dcontent_c, positions grouped by row)  fp32 (U, k d), deterministic, no atomics
        content_c  = table[row_index[c]] (a torch gather)  ->  dqk[c] = sense_dqk(qk[c], content_c, dout[c], lse[c])
    dtable is rounded to the table's dtype once, at the end.  The grouping is one stable sort and one searchsorted per
    chunk, on the device.  The sum over the chunks is in ascending chunk order, so the result is the same bits in every
    run; a different `chunk_samples` associates the sum differently."""

    @staticmethod
    def forward(ctx, qk, table, row_index, softmax_scale, chunk_samples):
        scale = softmax_scale or qk.shape[-1] ** -0.5
        row_index = row_index.to(torch.int32)
        lse = sense_lse(qk, scale)
        out = sense_mix_gather(qk, table, row_index, scale, lse=lse)
        ctx.save_for_backward(qk, table, row_index, lse)
        ctx.scale = scale
        ctx.chunk_samples = max(1, int(chunk_samples))
        return out

    @staticmethod
    def backward(ctx, dout):
        qk, table, row_index, lse = ctx.saved_tensors
        dout = dout.contiguous()
        (b, s, _, k, dk), (u, _, d) = qk.shape, table.shape
        step = min(ctx.chunk_samples, b)
        want_qk, want_table = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        dqk = torch.empty_like(qk) if want_qk else None
        dtable = torch.empty((u, k * d), dtype=torch.float32, device=table.device) if want_table else None
        dc_buf = torch.empty((step, s, k, d), dtype=table.dtype, device=table.device) if want_table else None
        c_buf = torch.empty((step * s, k * d), dtype=table.dtype, device=table.device) if want_qk else None
        flat_table = table.view(u, k * d)
        for n, b0 in enumerate(range(0, b, step)):
            sl = slice(b0, min(b0 + step, b))
            c = sl.stop - sl.start
            if want_table:
                dcontent = sense_mix_dc(qk[sl], dout[sl], lse[sl], ctx.scale, table, out=dc_buf[:c])
                order, seg_begin = row_segments(row_index[sl], u)
                segment_sum_rows(dcontent.view(c * s, k * d), order, seg_begin, dtable, accumulate=n > 0)
            if want_qk:
                content = torch.index_select(flat_table, 0, row_index[sl].reshape(-1), out=c_buf[:c * s])
                sense_dqk(qk[sl], content.view(c, s, k, d), dout[sl], lse[sl], ctx.scale, out=dqk[sl])
        return dqk, (dtable.to(table.dtype).view(u, k, d) if want_table else None), None, None, None


SENSE_TABLE_TRAIN_CHUNK_SAMPLES = 8     # samples per chunk of SenseMixGatherFn's backward: a guess, NOT measured


def sense_mix_gather_autograd(qk, table, row_index, softmax_scale=None, chunk_samples=SENSE_TABLE_TRAIN_CHUNK_SAMPLES):
    """sense_mix_gather that records a backward when gradients are enabled (training), the plain kernel otherwise.  Shapes
    its backward does not take (sense_mix_gather_train_supported) raise: callers choose the per-position order for them."""
    if torch.is_grad_enabled() and (qk.requires_grad or table.requires_grad):
        _require_cuda(qk, table, row_index)
        if not sense_mix_gather_train_supported(qk, table, qk.shape[1]):
            raise RuntimeError('bp_hip.sense_mix_gather_autograd: ' + sense_mix_gather_train_limits(qk, table, qk.shape[1]))
        return SenseMixGatherFn.apply(qk, table, row_index, softmax_scale, chunk_samples)
    return sense_mix_gather(qk, table, row_index.to(torch.int32), softmax_scale)


class SenseAlphaFn(torch.autograd.Function):
    """Differentiable bp_sense_alpha: backward = bp_softmax_bwd_causal + the two thin GEMMs."""

    @staticmethod
    def forward(ctx, qk, softmax_scale):
        scale = softmax_scale or qk.shape[-1] ** -0.5
        alpha = sense_alpha(qk, scale)
        ctx.save_for_backward(qk, alpha)
        ctx.scale = scale
        return alpha

    @staticmethod
    def backward(ctx, dalpha):
        qk, alpha = ctx.saved_tensors
        return _scores_backward(qk, alpha, dalpha.contiguous().clone(), ctx.scale), None


def sense_alpha_autograd(qk, softmax_scale=None):
    if torch.is_grad_enabled() and qk.requires_grad:
        return SenseAlphaFn.apply(qk, softmax_scale)
    return sense_alpha(qk, softmax_scale)


LN_BWD_WS_ROWS = 1024


def add_layer_norm_bwd_supported(x0_dtype, cols):
    return x0_dtype in (torch.float16, torch.bfloat16, torch.float32) and cols % 4 == 0 and cols <= 2048


def add_layer_norm_bwd(dz, dx_in, x, weight, eps, want_dx1, dropout_p=0.0, rng_state=None, rowscale=None, colscale=None,
                       x0=None):
    """Backward of add_layer_norm: (dx0 in dz's dtype, dx1 in x's dtype or None, dweight, dbias[, dcolscale]).
    dz (..., cols) in the forward's x0 / z dtype; dx_in gradient of the residual output (x's dtype) or None; x
    the summed stream the forward normalised (fp32 or dz's dtype).  With dropout, (dropout_p, rng_state) are the
    forward's: dx0 passes the regenerated mask and the 1 / (1 - p) scale.  rowscale / colscale: the forward's; with a
    colscale the forward's x0 is needed too and dcolscale is appended.  Replaces dropout_add_ln_bwd
    (flash_attn/ops/layer_norm.py:27-52)."""
    _require_cuda(dz, dx_in, x, weight, x0)
    cols = dz.shape[-1]
    dzc, xc = dz.contiguous(), x.contiguous()
    dxc = dx_in.contiguous() if dx_in is not None else None
    if xc.dtype not in (torch.float32, dzc.dtype) or (dxc is not None and dxc.dtype != xc.dtype):
        raise RuntimeError('bp_hip.add_layer_norm_bwd: x / dx_in must be fp32 or dz\'s dtype, and agree')
    if float(dropout_p) > 0.0 and rng_state is None:
        raise RuntimeError('bp_hip.add_layer_norm_bwd: dropout_p > 0 needs the rng_state the forward used')
    dropout_p, rng_state, rng_ptr = _dropout_args(dropout_p, rng_state, dz.device)
    rowscale, colscale = _ln_scales(dzc, weight, rowscale, colscale)
    x0c = None
    if colscale is not None:
        if x0 is None or x0.shape != dz.shape or x0.dtype != dz.dtype:
            raise RuntimeError('bp_hip.add_layer_norm_bwd: the gradient of colscale needs the forward\'s x0')
        x0c = x0.contiguous()
    code_dt, _ = _ln_16bit_code(dzc, xc, weight)
    rows = dzc.numel() // cols
    dx0 = torch.empty_like(dzc)
    dx1 = torch.empty_like(xc) if want_dx1 else None
    dw, db = torch.empty_like(weight), torch.empty_like(weight)
    dcs = torch.empty_like(weight) if colscale is not None else None
    ws = torch.empty(int(lib().bp_ln_bwd_ws_floats(cols, int(colscale is not None))), dtype=torch.float32, device=dz.device)
    _call('bp_dropout_add_layer_norm_scaled_bwd', dz.device,
          dzc.data_ptr(), dxc.data_ptr() if dxc is not None else None, xc.data_ptr(),
          x0c.data_ptr() if x0c is not None else None, weight.data_ptr(),
          rowscale.data_ptr() if rowscale is not None else None, colscale.data_ptr() if colscale is not None else None,
          dx0.data_ptr(), dx1.data_ptr() if dx1 is not None else None, dw.data_ptr(), db.data_ptr(),
          dcs.data_ptr() if dcs is not None else None, ws.data_ptr(), ws.numel(), rows, cols, float(eps), code_dt,
          int(dzc.dtype == torch.float32), int(xc.dtype == torch.float32), int(weight.dtype == torch.float32),
          dropout_p, rng_ptr)
    return (dx0, dx1, dw, db) if colscale is None else (dx0, dx1, dw, db, dcs)


def _xent_dtype(t):
    code = {torch.float16: 0, torch.bfloat16: 1, torch.float32: 2}.get(t.dtype)
    if code is None:
        raise RuntimeError(f'bp_hip: cross entropy takes fp16 / bf16 / fp32 logits, got {t.dtype}')
    return code


def xentropy_fwd(logits, labels, smoothing=0.0, total_classes=-1):
    """(losses, lse), both fp32 (rows,): the reference's xentropy_cuda_lib.forward
    (flash_attn/losses/cross_entropy.py:37,54).  logits (rows, cols), last dim contiguous; labels int64."""
    _require_cuda(logits, labels)
    if logits.dim() != 2 or logits.stride(1) != 1 or labels.shape != (logits.shape[0],):
        raise RuntimeError('bp_hip.xentropy_fwd: logits (rows, cols) with unit last stride, labels (rows,)')
    labels = labels.to(torch.int64).contiguous()
    rows, cols = logits.shape
    losses = torch.empty(rows, dtype=torch.float32, device=logits.device)
    lse = torch.empty(rows, dtype=torch.float32, device=logits.device)
    _call('bp_xentropy_fwd', logits.device, logits.data_ptr(), labels.data_ptr(), losses.data_ptr(), lse.data_ptr(),
          rows, cols, logits.stride(0), float(smoothing), int(total_classes), _xent_dtype(logits))
    return losses, lse


def xentropy_bwd(grad_losses, logits, lse, labels, smoothing=0.0, inplace=False, total_classes=-1):
    """d loss / d logits in the logits' dtype; `inplace` overwrites `logits` (upstream's inplace_backward,
    cross_entropy.py:103-105)."""
    _require_cuda(grad_losses, logits, lse, labels)
    rows, cols = logits.shape
    grad = logits if inplace else torch.empty_like(logits)
    g = grad_losses.to(torch.float32).contiguous()
    labels = labels.to(torch.int64).contiguous()
    _call('bp_xentropy_bwd', logits.device, g.data_ptr(), logits.data_ptr(), lse.data_ptr(), labels.data_ptr(),
          grad.data_ptr(), rows, cols, logits.stride(0), grad.stride(0), float(smoothing), int(total_classes),
          _xent_dtype(logits))
    return grad


def bias_gelu_supported(x):
    """Shapes / dtypes bp_bias_gelu_* and bp_column_sum take (callers use the torch expressions otherwise)."""
    return x.is_cuda and x.dtype in (torch.float16, torch.bfloat16) and x.shape[-1] % 8 == 0 and x.numel() > 0


def _rows_cols(x):
    if x.stride(-1) != 1 or not x.is_contiguous():
        raise RuntimeError('bp_hip: bias/GELU kernels take contiguous (rows, cols) tensors')
    return x.numel() // x.shape[-1], x.shape[-1]


def bias_gelu_fwd(x, bias=None, save_pre=False, out=None):
    """y = gelu_tanh(x + bias) for a contiguous 16-bit (..., cols) tensor; returns (y, pre) where pre = x + bias
    (16-bit) when save_pre -- without a bias, pre IS x.  `out` may be x itself (in place).  C ABI bp_bias_gelu_fwd:
    the elementwise half of the reference's `linear_gelu_forward` (flash_attn/ops/fused_dense.py:220)."""
    _require_cuda(x, bias, out)
    rows, cols = _rows_cols(x)
    if bias is not None and (bias.shape != (cols,) or bias.dtype != x.dtype or not bias.is_contiguous()):
        raise RuntimeError('bp_hip.bias_gelu_fwd: bias must be a contiguous (cols,) tensor of x\'s dtype')
    y = torch.empty_like(x) if out is None else out
    pre = torch.empty_like(x) if (save_pre and bias is not None) else None
    _call('bp_bias_gelu_fwd', x.device, x.data_ptr(), bias.data_ptr() if bias is not None else None,
          pre.data_ptr() if pre is not None else None, y.data_ptr(), rows, cols, _dtype_code(x))
    return y, (pre if pre is not None else (x if save_pre else None))


def _bias_grad_ws(rows, cols, device):
    return torch.empty(int(lib().bp_bias_grad_ws_floats(rows, cols)), dtype=torch.float32, device=device)


def bias_gelu_bwd(grad, pre, bias_grad_dtype=None, inplace=False):
    """(dpre, dbias): dpre = grad * gelu_tanh'(pre) in grad's dtype (written over `grad` when inplace) and, when
    bias_grad_dtype is given (fp32 or grad's dtype), dbias = column sums of dpre -- one pass over the two tensors, the
    reference's `bias_gelu_linear_dgrad_bgrad` epilogue (flash_attn/ops/fused_dense.py:290) minus the GEMM."""
    _require_cuda(grad, pre)
    rows, cols = _rows_cols(grad)
    if pre.shape != grad.shape or pre.dtype != grad.dtype or not pre.is_contiguous():
        raise RuntimeError('bp_hip.bias_gelu_bwd: pre must match grad')
    dpre = grad if inplace else torch.empty_like(grad)
    dbias = ws = None
    if bias_grad_dtype is not None:
        if bias_grad_dtype not in (torch.float32, grad.dtype):
            raise RuntimeError('bp_hip.bias_gelu_bwd: bias gradient dtype must be fp32 or grad\'s dtype')
        dbias = torch.empty(cols, dtype=bias_grad_dtype, device=grad.device)
        ws = _bias_grad_ws(rows, cols, grad.device)
    _call('bp_bias_gelu_bwd', grad.device, grad.data_ptr(), pre.data_ptr(), dpre.data_ptr(),
          dbias.data_ptr() if dbias is not None else None, ws.data_ptr() if ws is not None else None, rows, cols,
          _dtype_code(grad), int(bias_grad_dtype == torch.float32))
    return dpre, dbias


def column_sum(grad, out_dtype=None):
    """dbias (cols,) = sum over the rows of a contiguous 16-bit (..., cols) tensor, deterministic (C ABI
    bp_column_sum): the bias-gradient half of the reference's `linear_bias_wgrad` (fused_dense.py:66,281)."""
    _require_cuda(grad)
    rows, cols = _rows_cols(grad)
    out_dtype = out_dtype or grad.dtype
    if out_dtype not in (torch.float32, grad.dtype):
        raise RuntimeError('bp_hip.column_sum: output dtype must be fp32 or grad\'s dtype')
    dbias = torch.empty(cols, dtype=out_dtype, device=grad.device)
    ws = _bias_grad_ws(rows, cols, grad.device)
    _call('bp_column_sum', grad.device, grad.data_ptr(), dbias.data_ptr(), ws.data_ptr(), rows, cols, _dtype_code(grad),
          int(out_dtype == torch.float32))
    return dbias


class GraphedForward:
    """One forward of `module` captured in a HIP graph (torch.cuda.CUDAGraph -> hipGraph) and replayed:
    for launch-bound shapes (Backpack-Micro, B=4, S=128: ~100 launches of ~20 us each) replay is 4x
    faster than eager launching; at the headline shape the kernels are long and it changes nothing.
    Every C-ABI launch of this package goes to torch's current stream, so it is captured like a torch op.

        fwd = bp_hip.GraphedForward(model, example_ids)     # static shapes
        logits = fwd(ids)                                   # copies ids into the static input, replays
    The returned tensor is the graph's static output buffer (overwritten by the next call).
    """

    def __init__(self, module, example_input, select=lambda out: getattr(out, 'logits', out)):
        self.static_in = example_input.clone()
        self.select = select
        # caches a module keeps OUTSIDE the graph (the Backpack model's whole-vocabulary sense table): refreshed in place
        # in front of every replay, so in-place weight updates reach the replays as they reach the captured kernels
        self.refresh = getattr(module, 'refresh_inference_caches', None)
        side = torch.cuda.Stream(device=example_input.device)
        side.wait_stream(torch.cuda.current_stream(example_input.device))
        with torch.cuda.stream(side), torch.no_grad():
            for _ in range(2):              # warm-up outside capture (lazy inits, workspace allocations)
                module(self.static_in)
        torch.cuda.current_stream(example_input.device).wait_stream(side)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph), torch.no_grad():
            self.static_out = select(module(self.static_in))
        # The captured kernels hold the ADDRESS of such a cache.  Pin its storage (BackpackModel.train() would otherwise
        # free the table, and the refresh after the next eval() would build it somewhere else) and remember it: a replay
        # whose refresh did not land in this storage is refused instead of reading a freed block.
        self._pinned = []
        for m in module.modules():
            if hasattr(m, 'pin_sense_table') and m.sense_table_rows(stale_too=True) is not None:
                m.pin_sense_table()
                self._pinned.append((m, m.sense_table_rows(stale_too=True)))
        self.module = module

    def __call__(self, x):
        if self.module.training and self._pinned:
            raise RuntimeError('bp_hip.GraphedForward: the graph was captured in eval mode with the cached sense table; '
                               'call module.eval() before replaying it')
        self.static_in.copy_(x)
        if self.refresh is not None:
            with torch.no_grad():
                self.refresh()
        for m, table in self._pinned:
            now = m.sense_table_rows()             # None: dropped, or stale and not refreshed
            if now is None or now.data_ptr() != table.data_ptr():
                raise RuntimeError('bp_hip.GraphedForward: the sense table the graph reads was replaced or could not be '
                                   'refreshed in place; capture a new GraphedForward')
        self.graph.replay()
        return self.static_out


# ---- KV-cached decoding (C ABI bp_flash_decode / bp_sense_decode{,_weighted} / bp_sense_rows_dot) ---------------------------------------------------

def _decode_ws(floats, device):
    # fresh per call, like the other workspaces: the caching allocator hands it back once the stream has used it, and a
    # captured graph keeps its own block
    return torch.empty((max(int(floats), 4),), dtype=torch.float32, device=device)


def flash_decode_supported(q, kv_cache):
    """Whether bp_flash_decode takes these operands: 16-bit CUDA tensors, head_dim % 8 == 0 and <= 128, 16-byte
    friendly layouts (include/bp_hip.h)."""
    if not (q.is_cuda and kv_cache.is_cuda) or q.dtype not in (torch.float16, torch.bfloat16) or kv_cache.dtype != q.dtype:
        return False
    d = q.shape[-1]
    return d % 8 == 0 and d <= 128 and kv_cache.dim() == 5 and _vec16(q, kv_cache)


def flash_decode(q, k_new, v_new, kv_cache, cache_seqlens, softmax_scale=None, out=None, return_lse=False):
    """One decode step of trunk attention against the reference's KV cache.

    q, k_new, v_new (B, H, D) 16-bit; kv_cache (B, max_seqlen, 2, H, D) (already offset to the batch rows of this call);
    cache_seqlens (B,) int32 on the device: cached positions of every sample BEFORE this token.  Writes k_new / v_new into
    cache row cache_seqlens[b] and returns out (B, H, D) = softmax(scale q K[0..L]^T) V[0..L] (and the fp32 (B, H) LSE with
    return_lse).  The lengths are not advanced; the host never reads them."""
    _require_cuda(q, k_new, v_new, kv_cache, cache_seqlens)
    if q.dim() != 3 or k_new.shape != q.shape or v_new.shape != q.shape:
        raise RuntimeError('bp_hip.flash_decode: q, k_new, v_new must be (B, H, D) of one shape')
    b, h, d = q.shape
    if kv_cache.dim() != 5 or kv_cache.shape[0] != b or kv_cache.shape[2] != 2 or tuple(kv_cache.shape[3:]) != (h, d):
        raise RuntimeError(f'bp_hip.flash_decode: kv_cache must be (B, max_seqlen, 2, H, D) = ({b}, *, 2, {h}, {d}), '
                           f'got {tuple(kv_cache.shape)}')
    if k_new.dtype != q.dtype or v_new.dtype != q.dtype or kv_cache.dtype != q.dtype:
        raise RuntimeError('bp_hip.flash_decode: q, k_new, v_new and kv_cache dtypes differ')
    if cache_seqlens.shape != (b,) or cache_seqlens.dtype != torch.int32 or not cache_seqlens.is_contiguous():
        raise RuntimeError('bp_hip.flash_decode: cache_seqlens must be a contiguous (B,) int32 tensor')
    scale = softmax_scale or d ** -0.5
    max_s = kv_cache.shape[1]
    if out is None:
        out = torch.empty((b, h, d), dtype=q.dtype, device=q.device)
    lse = torch.empty((b, h), dtype=torch.float32, device=q.device) if return_lse else None
    ws = _decode_ws(lib().bp_flash_decode_ws_floats(b, h, d, max_s), q.device)
    _call('bp_flash_decode', q.device,
          q.data_ptr(), k_new.data_ptr(), v_new.data_ptr(), kv_cache.data_ptr(), cache_seqlens.data_ptr(),
          out.data_ptr(), lse.data_ptr() if lse is not None else None, ws.data_ptr(), ws.numel(),
          b, h, d, max_s, q.stride(0), q.stride(1), k_new.stride(0), k_new.stride(1), v_new.stride(0), v_new.stride(1),
          kv_cache.stride(0), kv_cache.stride(1), kv_cache.stride(2), kv_cache.stride(3),
          out.stride(0), out.stride(1), h, float(scale), _dtype_code(q))
    return (out, lse) if return_lse else out


SENSE_DECODE_MAX_SENSES = 64
SENSE_DECODE_MAX_DOUT = 2048


def sense_decode_supported(q, k_cache, table):
    """Whether bp_sense_decode takes these operands: 16-bit CUDA tensors, d_k % 8 == 0 and <= SENSE_MAX_DK, at most 64
    senses, d_out % 8 == 0 and <= 2048, 16-byte friendly layouts."""
    if not (q.is_cuda and k_cache.is_cuda and table.is_cuda) or q.dtype not in (torch.float16, torch.bfloat16):
        return False
    if k_cache.dtype != q.dtype or table.dtype != q.dtype or q.dim() != 3 or table.dim() != 3:
        return False
    k, dk, dout = q.shape[1], q.shape[2], table.shape[2]
    return (dk % 8 == 0 and dk <= SENSE_MAX_DK and 1 <= k <= SENSE_DECODE_MAX_SENSES and dout % 8 == 0
            and dout <= SENSE_DECODE_MAX_DOUT and _vec16(q, k_cache, table))


def _decode_key_weight_ok(key_weight, b, k, max_s):
    return (key_weight.is_cuda and key_weight.dtype == torch.float32 and tuple(key_weight.shape) == (b, k, max_s)
            and key_weight.stride(-1) == 1 and key_weight.stride(0) >= max_s and key_weight.stride(1) >= max_s)


def sense_decode_weighted_supported(q, k_cache, table, key_weight):
    """sense_decode_supported plus the weights' contract: fp32 (B, k, max_seqlen), unit stride along the positions."""
    return sense_decode_supported(q, k_cache, table) and k_cache.dim() == 4 \
        and _decode_key_weight_ok(key_weight, q.shape[0], q.shape[1], k_cache.shape[1])


def sense_decode(q, k_new, k_cache, table, row_index, new_row, cache_seqlens, softmax_scale=None, out=None,
                 key_weight=None):
    """One decode step of the Backpack sense contraction.

    q, k_new (B, k, d_k) 16-bit (the two halves of ContextSelfAttn.project for the new token); k_cache (B, max_seqlen, k,
    d_k); table (rows, k, d_out) sense vectors, read through row_index (B, max_seqlen) int32 (table form: token ids into the
    whole-vocabulary table; cache form: b * max_seqlen + j into a per-position content cache); new_row (B,) int32 the new
    position's row; cache_seqlens (B,) int32 cached positions before this one.  Appends k_new and new_row at position
    cache_seqlens[b] and returns (B, d_out) = sum_l sum_{j<=t} softmax_j(scale q_l . k_l(j)) table[row(j), l].

    key_weight (B, k, max_seqlen) fp32 or None: per-(sense, position) weights on the probabilities (they do not enter the
    softmax), entries [0, cache_seqlens[b]] read, the new position's included; C ABI bp_sense_decode_weighted."""
    _require_cuda(q, k_new, k_cache, table, row_index, new_row, cache_seqlens)
    if q.dim() != 3 or k_new.shape != q.shape:
        raise RuntimeError('bp_hip.sense_decode: q and k_new must be (B, k, d_k) of one shape')
    b, k, dk = q.shape
    if k_cache.dim() != 4 or k_cache.shape[0] != b or tuple(k_cache.shape[2:]) != (k, dk):
        raise RuntimeError(f'bp_hip.sense_decode: k_cache must be (B, max_seqlen, k, d_k) = ({b}, *, {k}, {dk}), '
                           f'got {tuple(k_cache.shape)}')
    max_s = k_cache.shape[1]
    if table.dim() != 3 or table.shape[1] != k:
        raise RuntimeError('bp_hip.sense_decode: table must be (rows, k, d_out)')
    if k_new.dtype != q.dtype or k_cache.dtype != q.dtype or table.dtype != q.dtype:
        raise RuntimeError('bp_hip.sense_decode: q, k_new, k_cache and table dtypes differ')
    if row_index.shape != (b, max_s) or row_index.dtype != torch.int32 or row_index.stride(-1) != 1:
        raise RuntimeError('bp_hip.sense_decode: row_index must be (B, max_seqlen) int32, unit stride along the sequence')
    for name, t in (('new_row', new_row), ('cache_seqlens', cache_seqlens)):
        if t.shape != (b,) or t.dtype != torch.int32 or not t.is_contiguous():
            raise RuntimeError(f'bp_hip.sense_decode: {name} must be a contiguous (B,) int32 tensor')
    dout = table.shape[2]
    scale = softmax_scale or dk ** -0.5
    if out is None:
        out = torch.empty((b, dout), dtype=q.dtype, device=q.device)
    ws = _decode_ws(lib().bp_sense_decode_ws_floats(b, k, dout, max_s), q.device)
    if key_weight is not None:
        if not _decode_key_weight_ok(key_weight, b, k, max_s):
            raise RuntimeError(f'bp_hip.sense_decode: key_weight must be a float32 CUDA tensor of shape ({b}, {k}, {max_s}) '
                               'with unit stride along the positions')
        _call('bp_sense_decode_weighted', q.device,
              q.data_ptr(), k_new.data_ptr(), k_cache.data_ptr(), table.data_ptr(), row_index.data_ptr(),
              new_row.data_ptr(), cache_seqlens.data_ptr(), key_weight.data_ptr(), out.data_ptr(), ws.data_ptr(),
              ws.numel(), b, k, dk, dout, max_s, table.shape[0], q.stride(0), q.stride(1), k_new.stride(0),
              k_new.stride(1), k_cache.stride(0), k_cache.stride(1), k_cache.stride(2), table.stride(0), table.stride(1),
              row_index.stride(0), out.stride(0), key_weight.stride(0), key_weight.stride(1), float(scale),
              _dtype_code(q))
        return out
    _call('bp_sense_decode', q.device,
          q.data_ptr(), k_new.data_ptr(), k_cache.data_ptr(), table.data_ptr(), row_index.data_ptr(),
          new_row.data_ptr(), cache_seqlens.data_ptr(), out.data_ptr(), ws.data_ptr(), ws.numel(),
          b, k, dk, dout, max_s, table.shape[0], q.stride(0), q.stride(1), k_new.stride(0), k_new.stride(1),
          k_cache.stride(0), k_cache.stride(1), k_cache.stride(2), table.stride(0), table.stride(1),
          row_index.stride(0), out.stride(0), float(scale), _dtype_code(q))
    return out


def sense_rows_dot_supported(table, vec):
    """Whether bp_sense_rows_dot takes these operands: 16-bit CUDA tensors of one dtype, at most 64 senses, d_out % 8 == 0
    and <= 2048, 16-byte friendly layouts."""
    if not (table.is_cuda and vec.is_cuda) or table.dtype not in (torch.float16, torch.bfloat16) or vec.dtype != table.dtype:
        return False
    if table.dim() != 3 or vec.dim() != 2 or vec.shape[1] != table.shape[2]:
        return False
    k, dout = table.shape[1], table.shape[2]
    return 1 <= k <= SENSE_DECODE_MAX_SENSES and dout % 8 == 0 and dout <= SENSE_DECODE_MAX_DOUT and _vec16(table, vec)


def sense_rows_dot(table, row_index, new_row, cache_seqlens, vec, out):
    """out[b, l, j] = table[row(b, j), l, :] . vec[b, :] for j = 0 .. cache_seqlens[b], where row(b, j) = row_index[b, j] for
    the cached positions and new_row[b] for j = cache_seqlens[b] (C ABI bp_sense_rows_dot; the annealed intervention's
    running similarity sums).  table (rows, k, d_out) and vec (B, d_out) 16-bit; row_index (B, max_seqlen) int32 (only
    read); out (B, k, max_seqlen) fp32, unit stride along the positions, written in place at [0, cache_seqlens[b]] and
    returned.  The lengths stay on the device."""
    _require_cuda(table, row_index, new_row, cache_seqlens, vec, out)
    if table.dim() != 3 or vec.dim() != 2 or vec.shape[1] != table.shape[2] or vec.dtype != table.dtype:
        raise RuntimeError('bp_hip.sense_rows_dot: table must be (rows, k, d_out) and vec (B, d_out) of the same dtype')
    b, (k, dout) = vec.shape[0], table.shape[1:]
    if row_index.dim() != 2 or row_index.shape[0] != b or row_index.dtype != torch.int32 or row_index.stride(-1) != 1:
        raise RuntimeError('bp_hip.sense_rows_dot: row_index must be (B, max_seqlen) int32, unit stride along the sequence')
    max_s = row_index.shape[1]
    for name, t in (('new_row', new_row), ('cache_seqlens', cache_seqlens)):
        if t.shape != (b,) or t.dtype != torch.int32 or not t.is_contiguous():
            raise RuntimeError(f'bp_hip.sense_rows_dot: {name} must be a contiguous (B,) int32 tensor')
    if not _decode_key_weight_ok(out, b, k, max_s):
        raise RuntimeError(f'bp_hip.sense_rows_dot: out must be a float32 CUDA tensor of shape ({b}, {k}, {max_s}) with unit '
                           'stride along the positions')
    _call('bp_sense_rows_dot', table.device,
          table.data_ptr(), row_index.data_ptr(), new_row.data_ptr(), cache_seqlens.data_ptr(), vec.data_ptr(),
          out.data_ptr(), b, k, dout, max_s, table.shape[0], table.stride(0), table.stride(1), row_index.stride(0),
          vec.stride(0), out.stride(0), out.stride(1), _dtype_code(table))
    return out


# ---- token selection on the device (C ABI bp_pick_token, bp_pick_token_ctl, bp_pick_token_lim, bp_pick_token_lim_rows, bp_pick_token_phrases) ---------------------------------------------------------------------------------------------

_PICK_DTYPES = {torch.float16: 0, torch.bfloat16: 1, torch.float32: 2}


PICK_MAX_PHRASE_LEN = 64      # BP_PICK_MAX_PHRASE_LEN of include/bp_hip.h
PICK_MAX_PHRASES = 1024       # BP_PICK_MAX_PHRASES


def pack_phrases(phrases, device, what='phrases'):
    """A list of token-id lists as the (ids, offsets) pair of int32 tensors on `device` that bp_pick_token_phrases reads: phrase
    j is ids[offsets[j] : offsets[j + 1]].  An already packed pair passes through (checked for form, not read).  ValueError for
    an empty phrase, one longer than PICK_MAX_PHRASE_LEN, and more than PICK_MAX_PHRASES phrases."""
    if isinstance(phrases, tuple) and len(phrases) == 2 and all(isinstance(t, torch.Tensor) for t in phrases):   # a TUPLE
        ids, offsets = phrases
        if any(t.dim() != 1 or t.dtype != torch.int32 or not t.is_contiguous() for t in (ids, offsets)) or offsets.numel() < 1:
            raise RuntimeError(f'bp_hip.pick_token: packed {what} must be contiguous 1-d int32 tensors (ids, offsets)')
        if offsets.numel() - 1 > PICK_MAX_PHRASES:
            raise ValueError(f'bp_hip.pick_token: at most {PICK_MAX_PHRASES} {what}')
        return ids, offsets
    rows = [[int(t) for t in (ph.tolist() if isinstance(ph, torch.Tensor) else ph)] for ph in phrases]
    if len(rows) > PICK_MAX_PHRASES:
        raise ValueError(f'bp_hip.pick_token: at most {PICK_MAX_PHRASES} {what}')
    if any(not 1 <= len(r) <= PICK_MAX_PHRASE_LEN for r in rows):
        raise ValueError(f'bp_hip.pick_token: every one of {what} must hold 1 to {PICK_MAX_PHRASE_LEN} ids')
    offsets = [0]
    for r in rows:
        offsets.append(offsets[-1] + len(r))
    ids = torch.tensor([t for r in rows for t in r], dtype=torch.int32).to(device)
    return ids, torch.tensor(offsets, dtype=torch.int32).to(device)


def pick_form(repetition_penalty=1.0, eos_token_id=None, pad_token_id=None, min_length=0, finished=None,
              no_repeat_ngram_size=0, frequency_penalty=0.0, presence_penalty=0.0, penalty_begin=0, suppress_tokens=None,
              bad_words_ids=None, stop_sequences=None):
    """The C ABI entry pick_token calls for these options: 'phrases' (bp_pick_token_phrases) when bad_words_ids or stop_sequences
    is given, else 'rows' (bp_pick_token_lim_rows) when penalty_begin or min_length is a
    tensor (one value per row), else 'lim' (bp_pick_token_lim) when any limit is given, else 'ctl' (bp_pick_token_ctl) when any
    control is, else 'plain' (bp_pick_token).  A non-zero penalty_begin counts as a limit."""
    if bad_words_ids is not None or stop_sequences is not None:
        return 'phrases'
    if isinstance(penalty_begin, torch.Tensor) or isinstance(min_length, torch.Tensor):
        return 'rows'
    if not (no_repeat_ngram_size == 0 and frequency_penalty == 0.0 and presence_penalty == 0.0 and penalty_begin == 0
            and suppress_tokens is None):
        return 'lim'
    if not (repetition_penalty == 1.0 and eos_token_id is None and pad_token_id is None and min_length == 0
            and finished is None):
        return 'ctl'
    return 'plain'


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _pick_outputs(who, rows, logits, tokens, sequences, finished):
    """What pick_token and beam_pick share: the checks of logits (rows, vocab), tokens (allocated when None), sequences and
    finished, rows = B or groups * W.  Returns tokens and the arguments that place tokens and sequences in both ABIs."""
    if logits.dim() != 2 or logits.stride(1) != 1 or logits.dtype not in _PICK_DTYPES:
        raise RuntimeError(f'bp_hip.{who}: logits must be ({rows}, vocab) fp16 / bf16 / fp32 with a contiguous last dimension')
    n = logits.shape[0]
    if tokens is None:
        tokens = torch.empty((n,), dtype=torch.int64, device=logits.device)
    if tokens.dtype != torch.int64 or tokens.numel() != n or tokens.shape[0] != n:
        raise RuntimeError(f'bp_hip.{who}: tokens must be int64 with {rows} elements along its first dimension')
    if sequences is not None and (sequences.dim() != 2 or sequences.shape[0] != n or sequences.dtype != torch.int64
                                  or sequences.stride(1) != 1):
        raise RuntimeError(f'bp_hip.{who}: sequences must be ({rows}, cols) int64 with a contiguous last dimension')
    if finished is not None and (finished.shape != (n,) or finished.dtype != torch.int32 or not finished.is_contiguous()):
        raise RuntimeError(f'bp_hip.{who}: finished must be a contiguous ({rows},) int32 tensor')
    strides = (logits.stride(0), tokens.stride(0) if n > 1 else 1, sequences.stride(0) if sequences is not None else 0,
               sequences.shape[1] if sequences is not None else 0)
    return tokens, strides


def _pad_id(eos_token_id, pad_token_id):
    if pad_token_id is not None:
        return int(pad_token_id)
    return int(eos_token_id) if eos_token_id is not None else 0


def pick_token(logits, do_sample=False, temperature=1.0, top_k=0, top_p=1.0, rng_state=None, counters=None, tokens=None,
               sequences=None, return_stats=False, repetition_penalty=1.0, eos_token_id=None, pad_token_id=None, min_length=0,
               finished=None, no_repeat_ngram_size=0, frequency_penalty=0.0, presence_penalty=0.0, penalty_begin=0,
               suppress_tokens=None, bad_words_ids=None, stop_sequences=None, ends=None, reasons=None):
    """The next token of every row of `logits` (B, vocab) fp16 / bf16 / fp32 (any row stride), chosen on the device by one
    launch that reads no host value (legal inside a HIP-graph capture): argmax (lowest index of the maximum, NaN largest),
    or with do_sample a draw after temperature, top-k (ties kept) and top-p -- the contract is in include/bp_hip.h.

    rng_state: int64 {seed, offset} on the device (new_rng_state; drawn from torch's generator when None and do_sample);
    counters (B,) int32 on the device: the Philox counter of every row and the column of `sequences` (B, cols) int64 that
    also receives the pick (skipped outside [0, cols)); None: counter 0.  tokens: optional int64 output with B elements
    (any stride along its first dimension), allocated when None.  Returns tokens, or (tokens, stats) with return_stats:
    stats (B, 4) fp32 = lowest kept scaled logit, log-sum-exp of the kept ones, kept count, the uniform u.

    repetition_penalty, eos_token_id, pad_token_id (default: eos_token_id), min_length, finished ((B,) int32 on the device,
    read and written) select bp_pick_token_ctl: tokens of the history sequences[b, :counters[b]] have their logit multiplied
    by the penalty (negative) or its reciprocal, the EOS entry is -inf while counters[b] < min_length, a row whose flag is
    set picks the pad, and a row that picks the EOS id has its flag set.  With all five at their defaults the call is
    bp_pick_token's, argument for argument.

    no_repeat_ngram_size, frequency_penalty, presence_penalty, penalty_begin, suppress_tokens (an int32 tensor on the device)
    select bp_pick_token_lim, the controlled pick with more limits: an id that would complete an n-gram the history already
    holds and every id of suppress_tokens count as -inf, and an id that occurs n > 0 times at the history positions >=
    penalty_begin loses frequency_penalty * n + presence_penalty.  With all of them at their defaults the call routes exactly as
    described above (pick_form is the rule).

    penalty_begin and min_length each take an int, or a contiguous (B,) int32 tensor on the device with one value per row
    (negative entries count as 0): a tensor selects bp_pick_token_lim_rows, the limited pick for rows that begin at different
    positions.  The tensors are not read on the host.

    bad_words_ids, stop_sequences (each a list of token-id lists, packed here once per call, or an already packed (ids,
    offsets) pair of int32 tensors on the device: pack_phrases) select bp_pick_token_phrases, the row-limited pick with phrases:
    the last id of a bad word is -inf while the row's history ends with the ids in front of it, and a row whose text behind
    penalty_begin ends with a stop sequence has its flag set (needs `sequences` and `finished`), once counters[b] >= min_length.
    ends, reasons: optional contiguous (B,) int32 tensors on the device, written for the rows this call finishes: counters[b] + 1,
    and 0 for the EOS id or 1 + the index of the stop sequence.  Both need one of the two lists."""
    per_row = [v for v in (penalty_begin, min_length) if isinstance(v, torch.Tensor)]
    form = pick_form(repetition_penalty, eos_token_id, pad_token_id, min_length, finished, no_repeat_ngram_size,
                     frequency_penalty, presence_penalty, penalty_begin, suppress_tokens, bad_words_ids, stop_sequences)
    if form != 'phrases' and (ends is not None or reasons is not None):
        raise RuntimeError('bp_hip.pick_token: ends and reasons need bad_words_ids or stop_sequences')
    ban = pack_phrases(bad_words_ids, logits.device, 'bad_words_ids') if bad_words_ids is not None else None
    stop = pack_phrases(stop_sequences, logits.device, 'stop_sequences') if stop_sequences is not None else None
    _require_cuda(logits, rng_state, counters, tokens, sequences, finished, suppress_tokens, *per_row, *(ban or ()), *(stop or ()),
                  ends, reasons)
    tokens, strides = _pick_outputs('pick_token', 'B', logits, tokens, sequences, finished)
    batch, vocab = logits.shape
    if do_sample and rng_state is None:
        rng_state = new_rng_state(logits.device)
    if rng_state is not None and (rng_state.dtype != torch.int64 or rng_state.numel() != 2 or not rng_state.is_contiguous()):
        raise RuntimeError('bp_hip.pick_token: rng_state must be a contiguous int64 tensor of 2 elements')
    if counters is not None and (counters.shape != (batch,) or counters.dtype != torch.int32 or not counters.is_contiguous()):
        raise RuntimeError('bp_hip.pick_token: counters must be a contiguous (B,) int32 tensor')
    if suppress_tokens is not None and (suppress_tokens.dim() != 1 or suppress_tokens.dtype != torch.int32
                                        or not suppress_tokens.is_contiguous()):
        raise RuntimeError('bp_hip.pick_token: suppress_tokens must be a contiguous 1-d int32 tensor')
    if any(v.shape != (batch,) or v.dtype != torch.int32 or not v.is_contiguous() for v in per_row):
        raise RuntimeError('bp_hip.pick_token: a per-row penalty_begin / min_length must be a contiguous (B,) int32 tensor')
    if any(v is not None and (v.shape != (batch,) or v.dtype != torch.int32 or not v.is_contiguous()) for v in (ends, reasons)):
        raise RuntimeError('bp_hip.pick_token: ends and reasons must be contiguous (B,) int32 tensors')
    stats = torch.empty((batch, 4), dtype=torch.float32, device=logits.device) if return_stats else None
    args = [logits.data_ptr(), tokens.data_ptr(), _ptr(sequences), _ptr(stats), _ptr(rng_state), _ptr(counters)]
    if form != 'plain':
        args.append(_ptr(finished))
    args += [batch, vocab, *strides, int(bool(do_sample)), float(temperature), int(top_k), float(top_p)]
    if form != 'plain':
        args += [float(repetition_penalty), -1 if eos_token_id is None else int(eos_token_id),
                 _pad_id(eos_token_id, pad_token_id), 0 if isinstance(min_length, torch.Tensor) else int(min_length)]
    if form in ('lim', 'rows', 'phrases'):
        n_suppress = suppress_tokens.numel() if suppress_tokens is not None else 0
        args += [int(no_repeat_ngram_size), float(frequency_penalty), float(presence_penalty),
                 0 if isinstance(penalty_begin, torch.Tensor) else int(penalty_begin),
                 suppress_tokens.data_ptr() if n_suppress else None, n_suppress]
    if form in ('rows', 'phrases'):
        args += [v.data_ptr() if isinstance(v, torch.Tensor) else None for v in (penalty_begin, min_length)]
    if form == 'phrases':
        for packed in (ban, stop):
            n = packed[1].numel() - 1 if packed is not None else 0
            args += [packed[0].data_ptr(), packed[1].data_ptr(), n, packed[0].numel()] if n > 0 else [None, None, 0, 0]
        args += [_ptr(ends), _ptr(reasons)]
    _call({'plain': 'bp_pick_token', 'ctl': 'bp_pick_token_ctl', 'lim': 'bp_pick_token_lim', 'rows': 'bp_pick_token_lim_rows',
           'phrases': 'bp_pick_token_phrases'}[form], logits.device, *args, _PICK_DTYPES[logits.dtype])
    return (tokens, stats) if return_stats else tokens


# ---- beam search on the device (C ABI bp_beam_pick, bp_beam_copy_rows) ------------------------------------------------------------------------------------------------

_beam_ws = {}   # (device, groups, beam_width) -> workspace: one per shape, so a captured step keeps reading its own


def beam_pick(logits, beam_scores, parent, beam_width, finished=None, tokens=None, sequences=None, counters=None,
              eos_token_id=None, pad_token_id=None):
    """One beam-search step on the device (contract in include/bp_hip.h): logits (groups * W, vocab) fp16 / bf16 / fp32 (any
    row stride), beam_scores (groups * W,) fp32 and finished (groups * W,) int32 read and written, parent (groups * W,) int32
    written with the global row every slot continues.  tokens / sequences / counters as pick_token's.  Two launches that
    read no host value (legal inside a HIP-graph capture).  Returns tokens."""
    _require_cuda(logits, beam_scores, parent, finished, tokens, sequences, counters)
    tokens, strides = _pick_outputs('beam_pick', 'groups * W', logits, tokens, sequences, finished)
    rows, vocab = logits.shape
    beam_width = int(beam_width)
    if beam_width < 1 or rows % beam_width:
        raise RuntimeError('bp_hip.beam_pick: the rows of logits must be a multiple of beam_width >= 1')
    groups = rows // beam_width
    for name, t, dtype in (('beam_scores', beam_scores, torch.float32), ('parent', parent, torch.int32),
                           ('counters', counters, torch.int32)):
        if t is not None and (t.shape != (rows,) or t.dtype != dtype or not t.is_contiguous()):
            raise RuntimeError(f'bp_hip.beam_pick: {name} must be a contiguous (groups * W,) {dtype} tensor')
    key = (logits.device, groups, beam_width)
    ws = _beam_ws.get(key)
    if ws is None:
        floats = lib().bp_beam_pick_ws_floats(groups, beam_width)
        ws = _beam_ws[key] = torch.empty((max(int(floats), 4),), dtype=torch.float32, device=logits.device)
    _call('bp_beam_pick', logits.device,
          logits.data_ptr(), beam_scores.data_ptr(), _ptr(finished), parent.data_ptr(), tokens.data_ptr(), _ptr(sequences),
          _ptr(counters), ws.data_ptr(), ws.numel(), groups, beam_width, vocab, *strides,
          -1 if eos_token_id is None else int(eos_token_id), _pad_id(eos_token_id, pad_token_id), _PICK_DTYPES[logits.dtype])
    return tokens


BEAM_COPY_MAX_SETS = 32


def beam_copy_rows(tensors, parent, lengths, first_position):
    """Rows r with parent[r] != r of every tensor take positions [first_position, lengths[r]) of row parent[r], in ONE
    launch for all tensors (at most 32).  Each tensor is (rows, positions, ...) with everything behind the first
    dimension contiguous; parent, lengths (rows,) int32 on the device.  The caller guarantees
    parent[parent[r]] == parent[r] (beam_pick's slot rule does).  The tensors' addresses are read now: a captured graph
    keeps copying THESE buffers."""
    tensors = list(tensors)
    _require_cuda(parent, lengths, *tensors)
    if not tensors or len(tensors) > BEAM_COPY_MAX_SETS:
        raise RuntimeError(f'bp_hip.beam_copy_rows: between 1 and {BEAM_COPY_MAX_SETS} tensors, got {len(tensors)}')
    rows = parent.shape[0]
    for name, t in (('parent', parent), ('lengths', lengths)):
        if t.shape != (rows,) or t.dtype != torch.int32 or not t.is_contiguous():
            raise RuntimeError(f'bp_hip.beam_copy_rows: {name} must be a contiguous (rows,) int32 tensor')
    for t in tensors:
        if t.dim() < 2 or t.shape[0] != rows or not t[0].is_contiguous():
            raise RuntimeError('bp_hip.beam_copy_rows: every tensor must be (rows, positions, ...), contiguous behind the rows')
    n = len(tensors)
    bases = (ctypes.c_void_p * n)(*[t.data_ptr() for t in tensors])
    strides = (ctypes.c_int64 * n)(*[t.stride(0) * t.element_size() for t in tensors])
    pos_bytes = (ctypes.c_int64 * n)(*[t[0, 0].numel() * t.element_size() for t in tensors])
    _call('bp_beam_copy_rows', parent.device, bases, strides, pos_bytes, n, parent.data_ptr(), lengths.data_ptr(), rows,
          int(first_position), min(t.shape[1] for t in tensors))


# ---- packed rows into padded buffers (C ABI bp_scatter_packed_rows) ----------------------------------------------------------------------------------------------------

SCATTER_MAX_SETS = 32
SCATTER_POSITIONS = 32      # positions one workgroup of the kernel owns (csrc/bp_kernels.h kScatterPositions)


def _dense_behind(t, lead):
    """Whether everything behind the first `lead` dimensions of `t` lies contiguously."""
    want = 1
    for size, stride in zip(reversed(t.shape[lead:]), reversed(t.stride()[lead:])):
        if size != 1 and stride != want:
            return False
        want *= size
    return True


def scatter_packed_rows(pairs, cu_seqlens, max_seqlen):
    """Row cu_seqlens[b] + j of every `src` lands at [b, j] of its `dst`, for j < min(len_b, max_seqlen, dst.shape[1]), in ONE
    launch for all pairs (at most 32); nothing else of a `dst` is written (contract in include/bp_hip.h).  `pairs`: a list of
    (src (total, ...), dst (batch, positions, ...)) with one dtype and one trailing shape per pair, everything behind src's
    first and dst's second dimension contiguous -- src may be a strided slice (qkv[:, 1:] of a (total, 3, H, D) tensor), dst
    a batch slice of a cache (cache[b0:b1]).  cu_seqlens (batch + 1,) int32 on the device is read there only: no host read,
    legal inside a HIP-graph capture.  The tensors' addresses are read now: a captured graph keeps copying THESE buffers."""
    pairs = [tuple(pair) for pair in pairs]
    _require_cuda(cu_seqlens, *[t for pair in pairs for t in pair])
    if not pairs or len(pairs) > SCATTER_MAX_SETS:
        raise RuntimeError(f'bp_hip.scatter_packed_rows: between 1 and {SCATTER_MAX_SETS} pairs, got {len(pairs)}')
    if cu_seqlens.dim() != 1 or cu_seqlens.numel() < 2 or cu_seqlens.dtype != torch.int32 or not cu_seqlens.is_contiguous():
        raise RuntimeError('bp_hip.scatter_packed_rows: cu_seqlens must be a contiguous (batch + 1,) int32 tensor')
    batch, total = cu_seqlens.numel() - 1, pairs[0][0].shape[0] if pairs[0][0].dim() else -1
    for src, dst in pairs:
        if src.dim() < 1 or dst.dim() != src.dim() + 1 or src.dtype != dst.dtype or src.shape[1:] != dst.shape[2:]:
            raise RuntimeError('bp_hip.scatter_packed_rows: a pair is src (total, ...) and dst (batch, positions, ...) of one '
                               'dtype and one trailing shape')
        if src.shape[0] != total or dst.shape[0] != batch or src.device != cu_seqlens.device or dst.device != src.device:
            raise RuntimeError('bp_hip.scatter_packed_rows: every src holds the same `total` rows, every dst `batch` rows, '
                               'all on the device of cu_seqlens')
        if not _dense_behind(src, 1) or not _dense_behind(dst, 2):
            raise RuntimeError('bp_hip.scatter_packed_rows: everything behind src\'s first and dst\'s second dimension '
                               'must be contiguous')
    n = len(pairs)

    def array(kind, values):
        return (kind * n)(*values)
    row_bytes = [math.prod(src.shape[1:]) * src.element_size() for src, _ in pairs]

    def stride_bytes(t, dim, single):      # the stride of a dimension of one entry says nothing: `single` stands in
        return t.stride(dim) * t.element_size() if t.shape[dim] > 1 else single
    _call('bp_scatter_packed_rows', cu_seqlens.device,
          array(ctypes.c_void_p, [src.data_ptr() for src, _ in pairs]),
          array(ctypes.c_int64, [stride_bytes(src, 0, rb) for (src, _), rb in zip(pairs, row_bytes)]),
          array(ctypes.c_void_p, [dst.data_ptr() for _, dst in pairs]),
          array(ctypes.c_int64, [stride_bytes(dst, 0, 0) for _, dst in pairs]),
          array(ctypes.c_int64, [stride_bytes(dst, 1, rb) for (_, dst), rb in zip(pairs, row_bytes)]),
          array(ctypes.c_int64, row_bytes), n, cu_seqlens.data_ptr(), batch, total, int(max_seqlen),
          min(dst.shape[1] for _, dst in pairs))


# ---- row extremes on the device (C ABI bp_row_extremes) ---------------------------------------------------------------------------------------------------------------

ROW_EXTREMES_MAX_N = 64


def row_extremes_supported(logits, n):
    """Whether bp_row_extremes takes this call: a (rows, cols) fp16 / bf16 / fp32 CUDA tensor with a contiguous last
    dimension and 1 <= n <= min(cols, 64)."""
    return (logits.is_cuda and logits.dim() == 2 and logits.dtype in _PICK_DTYPES
            and logits.shape[1] >= 1 and logits.stride(1) == 1 and (logits.shape[0] <= 1 or logits.stride(0) >= logits.shape[1])
            and 1 <= int(n) <= min(logits.shape[1], ROW_EXTREMES_MAX_N))


def row_extremes(logits, n, largest=True, smallest=True, out=None):
    """The n largest and / or the n smallest elements of every row of `logits` (rows, cols) fp16 / bf16 / fp32 (any row
    stride), in one launch that reads no host value (contract in include/bp_hip.h): elements are ordered by the integer key
    of their raw bits (-0 < +0, NaNs at the ends by sign), ties by ascending column.  Returns (top_val, top_idx, bot_val,
    bot_idx): fp32 values and int32 columns, (rows, n) each, largest / smallest first; None for an end not asked for.
    `out`: the same four (contiguous, or None) to write into instead of allocating."""
    _require_cuda(logits)
    n = int(n)
    if logits.dim() != 2 or logits.dtype not in _PICK_DTYPES or (logits.shape[1] > 0 and logits.stride(1) != 1):
        raise RuntimeError('bp_hip.row_extremes: logits must be (rows, cols) fp16 / bf16 / fp32 with a contiguous last dimension')
    rows, cols = logits.shape
    want = (largest, largest, smallest, smallest)
    dtypes = (torch.float32, torch.int32, torch.float32, torch.int32)
    if out is None:
        out = [torch.empty((rows, n), dtype=dt, device=logits.device) if w else None for w, dt in zip(want, dtypes)]
    else:
        out = [o if w else None for w, o in zip(want, out)]
        _require_cuda(*out)
        for o, dt in zip(out, dtypes):
            if o is not None and (o.shape != (rows, n) or o.dtype != dt or not o.is_contiguous()):
                raise RuntimeError(f'bp_hip.row_extremes: every output must be a contiguous ({rows}, {n}) fp32 / int32 tensor')
    _call('bp_row_extremes', logits.device, logits.data_ptr(), *[o.data_ptr() if o is not None else None for o in out],
          rows, cols, logits.stride(0) if rows > 1 else max(cols, logits.stride(0)), n, _PICK_DTYPES[logits.dtype])
    return tuple(out)


# ---- sense attribution on the device (C ABI bp_sense_attribute) -------------------------------------------------------------------------------------------------------

ATTRIBUTE_MAX_VECS = 4


def sense_attribute_supported(qk, table, row_index, vec):
    """Whether bp_sense_attribute takes these operands: qk (B, S, 2, k, d_k) and table (rows, k, d_out) 16-bit CUDA tensors of
    one dtype in 16-byte friendly layouts, k <= 64, d_k % 8 == 0 and <= 640, d_out % 8 == 0 and <= 2048, row_index (B, S)
    integers, vec (nq, nvec, d_out) with 1 <= nvec <= 4 and nq <= 65535."""
    if not (qk.is_cuda and table.is_cuda and row_index.is_cuda and vec.is_cuda):
        return False
    if qk.dtype not in (torch.float16, torch.bfloat16) or table.dtype != qk.dtype:
        return False
    if qk.dim() != 5 or qk.shape[2] != 2 or table.dim() != 3 or vec.dim() != 3 or row_index.dim() != 2:
        return False
    b, s, _, k, dk = qk.shape
    dout = table.shape[2]
    return (b >= 1 and s >= 1 and table.shape[0] >= 1 and table.shape[1] == k and tuple(row_index.shape) == (b, s)
            and 1 <= k <= SENSE_DECODE_MAX_SENSES and dk % 8 == 0 and 8 <= dk <= SENSE_MAX_DK
            and dout % 8 == 0 and 8 <= dout <= SENSE_DECODE_MAX_DOUT and vec.shape[2] == dout
            and 1 <= vec.shape[1] <= ATTRIBUTE_MAX_VECS and 1 <= vec.shape[0] <= 65535
            and _vec16(qk, table) and qk.stride(2) % 8 == 0)


def sense_attribute(qk, table, row_index, query_sample, query_pos, vec, scale, want_probs=False, out=None, probs=None):
    """The share of every (position, sense) pair in the dot product of a position's output with `vec` (C ABI
    bp_sense_attribute, contract in include/bp_hip.h): for query n = position query_pos[n] of sample query_sample[n],
      out[n, v, l, j] = p_j * table[row_index[b_n, j], l, :] . vec[n, v, :],  p = softmax_{j <= i_n}(scale q_l(i_n) . k_l(j)),
    exact zeros behind i_n; the probabilities stay fp32.  qk (B, S, 2, k, d_k) and table (rows, k, d_out) 16-bit;
    row_index (B, S) int32; query_sample / query_pos (nq,) int32 on the device (clamped there, never read by the host);
    vec (nq, nvec, d_out) fp32.  Returns (out (nq, nvec, k, S) fp32, probs (nq, k, S) fp32 or None).  `out` / `probs`:
    fp32 tensors of those shapes with unit stride along S to write into (any other strides) instead of allocating."""
    _require_cuda(qk, table, row_index, query_sample, query_pos, vec, out, probs)
    b, s, k, dk = _check_qk(qk)
    if table.dim() != 3 or table.shape[1] != k or table.dtype != qk.dtype or table.stride(-1) != 1:
        raise RuntimeError('bp_hip.sense_attribute: table must be (rows, k, d_out) of the dtype of qk, contiguous last dim')
    dout = table.shape[2]
    if tuple(row_index.shape) != (b, s) or row_index.dtype != torch.int32 or row_index.stride(-1) != 1:
        raise RuntimeError('bp_hip.sense_attribute: row_index must be (B, S) int32, unit stride along the sequence')
    if vec.dim() != 3 or vec.shape[2] != dout or vec.dtype != torch.float32:
        raise RuntimeError('bp_hip.sense_attribute: vec must be (nq, nvec, d_out) float32')
    nq, nvec = vec.shape[:2]
    for name, t in (('query_sample', query_sample), ('query_pos', query_pos)):
        if tuple(t.shape) != (nq,) or t.dtype != torch.int32 or not t.is_contiguous():
            raise RuntimeError(f'bp_hip.sense_attribute: {name} must be a contiguous ({nq},) int32 tensor')
    if vec.stride(2) != 1 or vec.stride(0) % 4 or vec.stride(1) % 4 or vec.data_ptr() % 16:
        vec = vec.contiguous()
    if out is None:
        out = torch.empty((nq, nvec, k, s), dtype=torch.float32, device=qk.device)
    elif tuple(out.shape) != (nq, nvec, k, s) or out.dtype != torch.float32 or out.stride(-1) != 1:
        raise RuntimeError(f'bp_hip.sense_attribute: out must be float32 ({nq}, {nvec}, {k}, {s}) with unit stride along S')
    if probs is None and want_probs:
        probs = torch.empty((nq, k, s), dtype=torch.float32, device=qk.device)
    elif probs is not None and (tuple(probs.shape) != (nq, k, s) or probs.dtype != torch.float32 or probs.stride(-1) != 1):
        raise RuntimeError(f'bp_hip.sense_attribute: probs must be float32 ({nq}, {k}, {s}) with unit stride along S')
    ws_floats = lib().bp_sense_attribute_ws_floats(nq, k)
    ws = torch.empty((max(ws_floats, 1),), dtype=torch.float32, device=qk.device)
    _call('bp_sense_attribute', qk.device,
          qk.data_ptr(), table.data_ptr(), row_index.data_ptr(), query_sample.data_ptr(), query_pos.data_ptr(),
          vec.data_ptr(), out.data_ptr(), probs.data_ptr() if probs is not None else None, ws.data_ptr(), ws.numel(),
          b, s, k, dk, dout, nq, nvec, table.shape[0],
          qk.stride(0), qk.stride(1), qk.stride(2), qk.stride(3), table.stride(0), table.stride(1), row_index.stride(0),
          vec.stride(0), vec.stride(1), out.stride(0), out.stride(1), out.stride(2),
          probs.stride(0) if probs is not None else 0, probs.stride(1) if probs is not None else 0,
          float(scale), _dtype_code(qk))
    return out, probs


# ---- sense similarity on the device (C ABI bp_sense_similarity) -------------------------------------------------------------------------------------------------------

SIMILARITY_MAX_QUERY_ROWS = 64
SIMILARITY_OUTPUTS = ('flat', 'min_pair', 'max_pair', 'min_all', 'max_all', 'per_sense')


def sense_similarity_supported(table, query):
    """Whether bp_sense_similarity takes these operands: table (rows, k, d) and query (nq, k, d) 16-bit CUDA tensors of one
    dtype in 16-byte friendly layouts, k a power of two <= 64, 1 <= nq and nq * k <= 64, d % 8 == 0 and 8 <= d <= 2048."""
    if not (table.is_cuda and query.is_cuda) or table.dtype not in (torch.float16, torch.bfloat16) or query.dtype != table.dtype:
        return False
    if table.dim() != 3 or query.dim() != 3 or tuple(query.shape[1:]) != tuple(table.shape[1:]):
        return False
    rows, k, d = table.shape
    nq = query.shape[0]
    return (rows >= 1 and 1 <= k <= SENSE_DECODE_MAX_SENSES and k & (k - 1) == 0 and nq >= 1
            and nq * k <= SIMILARITY_MAX_QUERY_ROWS and d % 8 == 0 and 8 <= d <= SENSE_DECODE_MAX_DOUT and _vec16(table, query))


def sense_similarity(table, query, cand_index=None, want=SIMILARITY_OUTPUTS, out=None):
    """The cosine measures of the sense vectors of nq query words against candidate words of `table`, in one launch that
    reads every candidate's rows once (C ABI bp_sense_similarity, contract in include/bp_hip.h).  table (rows, k, d) and
    query (nq, k, d) 16-bit; cand_index (ncand,) int32 on the device (clamped there, never read by the host) or None: the
    candidates are rows 0 .. rows - 1.  Returns a dict over `want` (names of SIMILARITY_OUTPUTS): fp32 (nq, ncand) each --
    'flat' the cosine of the concatenated senses, 'min_pair' / 'max_pair' over matched senses, 'min_all' / 'max_all' over all
    sense pairs -- and 'per_sense' (nq, k, ncand), the cosine of every matched sense.  `out`: a dict of fp32 tensors of those
    shapes with unit stride along the candidates (the (nq, ncand) ones sharing one query stride) to write into."""
    _require_cuda(table, query, cand_index)
    if table.dim() != 3 or query.dim() != 3 or tuple(query.shape[1:]) != tuple(table.shape[1:]) or query.dtype != table.dtype:
        raise RuntimeError('bp_hip.sense_similarity: table must be (rows, k, d) and query (nq, k, d) of the same dtype')
    rows, k, d = table.shape
    nq = query.shape[0]
    if cand_index is None:
        ncand = rows
    elif cand_index.dim() != 1 or cand_index.dtype != torch.int32 or not cand_index.is_contiguous():
        raise RuntimeError('bp_hip.sense_similarity: cand_index must be a contiguous (ncand,) int32 tensor')
    else:
        ncand = cand_index.shape[0]
    want = tuple(want)
    if not want or any(w not in SIMILARITY_OUTPUTS for w in want):
        raise RuntimeError(f'bp_hip.sense_similarity: want must name some of {SIMILARITY_OUTPUTS}')
    res = {}
    for name in want:
        shape = (nq, k, ncand) if name == 'per_sense' else (nq, ncand)
        if out is not None and out.get(name) is not None:
            t = out[name]
            _require_cuda(t)
            if tuple(t.shape) != shape or t.dtype != torch.float32 or (ncand > 1 and t.stride(-1) != 1):
                raise RuntimeError(f'bp_hip.sense_similarity: {name} must be float32 {shape} with unit stride along the candidates')
            res[name] = t
        else:
            res[name] = torch.empty(shape, dtype=torch.float32, device=table.device)
    pair = [res[n] for n in want if n != 'per_sense']
    o_qs = max([ncand] + [t.stride(0) for t in pair]) if nq > 1 else ncand
    if nq > 1 and any(t.stride(0) != o_qs for t in pair):
        raise RuntimeError('bp_hip.sense_similarity: the (nq, ncand) outputs must share one query stride')
    ps = res.get('per_sense')
    ps_gs = ps.stride(1) if ps is not None and k > 1 else ncand
    ps_qs = ps.stride(0) if ps is not None and nq > 1 else k * ps_gs
    _call('bp_sense_similarity', table.device, table.data_ptr(), cand_index.data_ptr() if cand_index is not None else None,
          query.data_ptr(), *[res[n].data_ptr() if n in res else None for n in SIMILARITY_OUTPUTS],
          ncand, k, d, nq, rows, table.stride(0), table.stride(1), query.stride(0), query.stride(1), o_qs, ps_qs, ps_gs,
          _dtype_code(table))
    return res


# ---- row scoring on the device (C ABI bp_score_rows) ------------------------------------------------------------------------------------------------------------------

SCORE_MAX_TARGETS = 8
SCORE_OUTPUTS = ('logprob', 'rank', 'lse', 'top1', 'entropy')
_SCORE_DTYPES = {'logprob': torch.float32, 'rank': torch.int32, 'lse': torch.float32, 'top1': torch.int32, 'entropy': torch.float32}


def score_rows(logits, targets, want=SCORE_OUTPUTS):
    """What an evaluation keeps of every row of `logits` (rows, cols) fp16 / bf16 / fp32 (any row stride, unit last stride),
    in one launch that reads the row once (C ABI bp_score_rows, contract in include/bp_hip.h).  targets: int64 (rows,) or
    (rows, M), 1 <= M <= 8; a target outside [0, cols) (an ignore_index) scores logprob 0 and rank -1.  Returns a dict over
    `want` (names of SCORE_OUTPUTS): 'logprob' fp32 and 'rank' int32 in the shape of `targets` (0-based, ties towards the lower
    id), 'lse' fp32, 'top1' int32 (the greedy token of pick_token) and 'entropy' fp32, (rows,) each."""
    _require_cuda(logits, targets)
    want = tuple(want)
    if not want or any(w not in SCORE_OUTPUTS for w in want):
        raise RuntimeError(f'bp_hip.score_rows: want must name some of {SCORE_OUTPUTS}')
    if logits.dim() != 2 or logits.dtype not in _PICK_DTYPES or logits.shape[1] < 1 or logits.stride(1) != 1:
        raise RuntimeError('bp_hip.score_rows: logits must be (rows, cols) fp16 / bf16 / fp32 with a contiguous last dimension')
    rows, cols = logits.shape
    if targets.dim() not in (1, 2) or targets.shape[0] != rows or targets.dtype != torch.int64:
        raise RuntimeError('bp_hip.score_rows: targets must be int64 (rows,) or (rows, M)')
    flat = targets.reshape(rows, -1).contiguous()
    m = flat.shape[1]
    if not 1 <= m <= SCORE_MAX_TARGETS:
        raise RuntimeError(f'bp_hip.score_rows: 1 .. {SCORE_MAX_TARGETS} targets per row, got {m}')
    res = {n: torch.empty(tuple(targets.shape) if n in ('logprob', 'rank') else (rows,), dtype=_SCORE_DTYPES[n], device=logits.device)
           for n in want}
    if rows == 0:
        return res
    _call('bp_score_rows', logits.device, logits.data_ptr(), flat.data_ptr(),
          *[res[n].data_ptr() if n in res else None for n in SCORE_OUTPUTS],
          rows, cols, m, logits.stride(0) if rows > 1 else max(cols, logits.stride(0)), m, m, _PICK_DTYPES[logits.dtype])
    return res


# ---- the record of a pick on the device (C ABI bp_pick_report) ---------------------------------------------------------------------------------------------------------

PICK_REPORT_MAX_TOP = 16
PICK_REPORT_RECORDS = ('logprob', 'rank', 'entropy', 'top_idx', 'top_logprob')
_REPORT_DTYPES = {'logprob': torch.float32, 'rank': torch.int32, 'entropy': torch.float32, 'top_idx': torch.int32,
                  'top_logprob': torch.float32}


def pick_report_supported(logits, n_top=0):
    """Whether bp_pick_report takes this call: a (rows >= 1, vocab >= 1) fp16 / bf16 / fp32 CUDA tensor with a contiguous last
    dimension and 0 <= n_top <= min(vocab, 16)."""
    return (logits.is_cuda and logits.dim() == 2 and logits.dtype in _PICK_DTYPES and logits.shape[0] >= 1
            and logits.shape[1] >= 1 and logits.stride(1) == 1 and (logits.shape[0] <= 1 or logits.stride(0) >= logits.shape[1])
            and 0 <= int(n_top) <= min(logits.shape[1], PICK_REPORT_MAX_TOP))


def pick_report(logits, tokens, counters, *, logprob=None, rank=None, entropy=None, top_idx=None, top_logprob=None):
    """The record of a pick, in one launch that reads no host value (C ABI bp_pick_report, contract in include/bp_hip.h; legal
    inside a HIP-graph capture): for every row b of `logits` (B, vocab) fp16 / bf16 / fp32 (any row stride), into column c =
    counters[b] of the records that are given -- logprob fp32, rank int32 and entropy fp32 (B, cols): the log-probability and the
    0-based rank of tokens[b] under the row and the row's entropy, as score_rows defines them; top_idx int32 and top_logprob fp32
    (B, cols, n), n <= 16: the n most likely tokens in pick_token's greedy order and their log-probabilities.  A row whose c
    lies outside [0, cols) is left alone; every other column too.  tokens: int64 with B elements (any stride along its first
    dimension, e.g. the (B, 1) input of the next decode step); counters: contiguous (B,) int32.  The records are views with a
    contiguous last dimension that share their width and ONE row stride (top_*: that stride times n), e.g. the leading
    columns of buffers as wide as the cache.  Returns None."""
    given = {'logprob': logprob, 'rank': rank, 'entropy': entropy, 'top_idx': top_idx, 'top_logprob': top_logprob}
    _require_cuda(logits, tokens, counters, *given.values())
    if logits.dim() != 2 or logits.dtype not in _PICK_DTYPES or logits.shape[0] < 1 or logits.shape[1] < 1 or logits.stride(1) != 1:
        raise RuntimeError('bp_hip.pick_report: logits must be (B, vocab) fp16 / bf16 / fp32 with a contiguous last dimension')
    batch, vocab = logits.shape
    if tokens.dtype != torch.int64 or tokens.numel() != batch or tokens.shape[0] != batch:
        raise RuntimeError('bp_hip.pick_report: tokens must be int64 with B elements along its first dimension')
    if counters.shape != (batch,) or counters.dtype != torch.int32 or not counters.is_contiguous():
        raise RuntimeError('bp_hip.pick_report: counters must be a contiguous (B,) int32 tensor')
    if all(v is None for v in given.values()):
        raise RuntimeError(f'bp_hip.pick_report: give at least one of {PICK_REPORT_RECORDS}')
    n_top, places = 0, set()
    for name, v in given.items():
        if v is None:
            continue
        top = name.startswith('top_')
        if v.dtype != _REPORT_DTYPES[name] or v.dim() != (3 if top else 2) or v.shape[0] != batch or v.shape[1] < 1:
            raise RuntimeError(f'bp_hip.pick_report: {name} must be {_REPORT_DTYPES[name]} (B, cols' + (', n)' if top else ')'))
        n = v.shape[2] if top else 1
        if top and (not 1 <= n <= min(vocab, PICK_REPORT_MAX_TOP) or n_top not in (0, n)):
            raise RuntimeError(f'bp_hip.pick_report: top_idx and top_logprob hold the same 1 .. min(vocab, {PICK_REPORT_MAX_TOP}) '
                               'entries per pick')
        if top:
            n_top = n
        cols = v.shape[1]
        row = v.stride(0) if batch > 1 else max(cols * n, v.stride(0))
        if v.stride(-1) != 1 or (top and cols > 1 and v.stride(1) != n) or row % n != 0:
            raise RuntimeError(f'bp_hip.pick_report: {name} must be dense behind its first dimension')
        places.add((cols, row // n if batch > 1 else None))
    widths = {c for c, _ in places}
    strides = {r for _, r in places if r is not None}
    if len(widths) != 1 or len(strides) > 1:
        raise RuntimeError('bp_hip.pick_report: the records must share their width and their row stride')
    rec_cols = widths.pop()
    rec_stride = strides.pop() if strides else rec_cols
    _call('bp_pick_report', logits.device, logits.data_ptr(), tokens.data_ptr(), counters.data_ptr(),
          *[_ptr(given[name]) for name in PICK_REPORT_RECORDS], batch, vocab,
          logits.stride(0) if batch > 1 else max(vocab, logits.stride(0)), tokens.stride(0) if batch > 1 else 1,
          rec_cols, rec_stride, n_top, _PICK_DTYPES[logits.dtype])


# ---- dense layers by a pinned hipBLASLt solution (C ABI bp_gemm_*): bp_hip/gemm.py ---------------------------------------------
from .gemm import GemmTable, linear, lm_head_chunk_rows   # noqa: E402,F401
