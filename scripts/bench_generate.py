"""Greedy decoding latency of Backpack-Small on the HIP path: the reference's growing-prefix loop (no KV cache upstream)
against generate(..., cg=True), one captured full-width forward replayed per token, and the KV-cached decode,
generate(..., kv_cache=True) eagerly and with cg=True (one captured decode step replayed per token; src/utils/generation.py).

    python scripts/bench_generate.py [--batch 1] [--prompt 16] [--max-length 128] [--model small] [--modes off,cached]
                                     [--legs full,kv]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'backpacks-flash-attn_amd')):
    sys.path.insert(0, p)
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=1)
    ap.add_argument('--prompt', type=int, default=16)
    ap.add_argument('--max-length', type=int, default=128)
    ap.add_argument('--model', default='small')
    ap.add_argument('--modes', default='off,cached', help='sense_table modes to run')
    ap.add_argument('--legs', default='full,kv', help='full: growing-prefix loop and its graph; kv: the KV-cached legs')
    a = ap.parse_args()
    from bench import MODELS
    from src.models.backpack import BackpackConfig, BackpackLMHeadModel
    dev = torch.device('cuda', 0)
    cfg = BackpackConfig(vocab_size=50257, n_positions=max(a.max_length, 128), scale_attn_by_inverse_layer_idx=True,
                         use_flash_attn=True, fused_bias_fc=True, fused_dense_gelu_dense=True, fused_dropout_add_ln=True,
                         pad_vocab_size_multiple=8, **MODELS[a.model])
    torch.manual_seed(0)
    model = BackpackLMHeadModel(cfg, device=dev, dtype=torch.bfloat16).eval()
    ids = torch.randint(0, 50257, (a.batch, a.prompt), device=dev)
    legs = []
    if 'full' in a.legs.split(','):
        legs += [('eager_loop', False, False), ('graph_replay', True, False)]
    if 'kv' in a.legs.split(','):
        legs += [('kv_cache_eager', False, True), ('kv_cache_graph', True, True)]
    for mode in a.modes.split(','):   # content network per position (the reference's order) / cached whole-vocabulary table
        model.transformer.sense_table_mode = mode
        res = dict(model=a.model, batch=a.batch, prompt=a.prompt, max_length=a.max_length,
                   new_tokens=a.max_length - 1 - a.prompt, sense_table=mode)
        outs = {}
        for key, cg, kv in legs:
            model.generate(ids, max_length=a.max_length, cg=cg, kv_cache=kv)      # warm-up (allocator, library handles)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            outs[key] = model.generate(ids, max_length=a.max_length, cg=cg, kv_cache=kv)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            res[key + '_ms'] = round(dt * 1e3, 1)
            res[key + '_ms_per_token'] = round(dt * 1e3 / res['new_tokens'], 3)
        # random weights: near-uniform logits, ties flip easily
        if 'eager_loop' in outs:
            res['tokens_equal_fraction'] = round((outs['eager_loop'] == outs['graph_replay']).float().mean().item(), 4)
        if 'kv_cache_eager' in outs:
            res['kv_tokens_equal_graph'] = bool(torch.equal(outs['kv_cache_eager'], outs['kv_cache_graph']))
            if 'eager_loop' in outs:
                res['kv_tokens_equal_fraction'] = round(
                    (outs['kv_cache_eager'] == outs['eager_loop']).float().mean().item(), 4)
        print(json.dumps(res), flush=True)

if __name__ == '__main__':
    main()
