"""Row scoring on the device against what it replaces, and against the bandwidth yardstick.

    python scripts/bench_scoring.py [--rows 16384] [--cols 50264] [--runs 5] [--batch 16] [--seq 1024] [--no-model]
                                    [--out profiles/scoring_bench.jsonl]

Three legs alternate in one process, --runs times each, on one chunk of (rows, cols) bf16 logits with drawn labels:
  score      bp_score_rows at M = 1, all five outputs
  xentropy   bp_xentropy_fwd: it reads the same bytes, so it is what the memory system allows (5.6 TB/s)
  torch      the composition bp_score_rows replaces: fp32 log_softmax, gather, argmax, comparison count, entropy
Per leg: every run's milliseconds (device events), the median, the minimum and the peak of the allocator above the inputs.
Then, unless --no-model, Backpack-Small at --batch x --seq tokens: evaluate_lm (src/utils/scoring.py) against lm_loss_chunked
(src/utils/perplexity.py), alternating, in tokens per second.  One JSON line per part goes to stdout and is appended to --out."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'backpacks-flash-attn_amd')):
    sys.path.insert(0, p)
import torch  # noqa: E402


def timed(fn):
    """(milliseconds on the device, allocator peak in bytes above what was live before the call)."""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    live = torch.cuda.memory_allocated()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    out = fn()
    stop.record()
    torch.cuda.synchronize()
    del out
    return start.elapsed_time(stop), torch.cuda.max_memory_allocated() - live


def alternate(legs, runs):
    """legs: name -> callable.  One untimed call each, then `runs` rounds over all legs in order."""
    for fn in legs.values():
        fn()
    ms, peak = {n: [] for n in legs}, {n: 0 for n in legs}
    for _ in range(runs):
        for name, fn in legs.items():
            t, p = timed(fn)
            ms[name].append(round(t, 4))
            peak[name] = max(peak[name], p)
    return ms, peak


def emit(line, path):
    text = json.dumps(line)
    print(text, flush=True)
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, 'a') as f:
            f.write(text + '\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=16384)
    ap.add_argument('--cols', type=int, default=50264)
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--seq', type=int, default=1024)
    ap.add_argument('--no-model', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'scoring_bench.jsonl'))
    a = ap.parse_args()
    import bp_hip
    dev = torch.device('cuda', 0)
    g = torch.Generator(device=dev).manual_seed(0)
    logits = (3.0 * torch.randn(a.rows, a.cols, device=dev, generator=g)).bfloat16()
    labels = torch.randint(0, a.cols, (a.rows,), device=dev, generator=g)

    def torch_composition():
        logp = torch.log_softmax(logits.float(), dim=-1)
        gold = logp.gather(1, labels[:, None])
        top1 = logits.argmax(dim=-1)
        rank = (logp > gold).sum(dim=-1)
        entropy = -(logp.exp() * logp).sum(dim=-1)
        return gold, top1, rank, entropy

    legs = {'score': lambda: bp_hip.score_rows(logits, labels), 'xentropy': lambda: bp_hip.xentropy_fwd(logits, labels),
            'torch': torch_composition}
    ms, peak = alternate(legs, a.runs)
    nbytes = logits.numel() * logits.element_size()
    line = {'bench': 'score_rows', 'rows': a.rows, 'cols': a.cols, 'dtype': 'bf16', 'targets': 1, 'runs': a.runs}
    for name in legs:
        line[f'{name}_ms_runs'] = ms[name]
        line[f'{name}_ms_median'] = round(statistics.median(ms[name]), 4)
        line[f'{name}_ms_min'] = min(ms[name])
        line[f'{name}_peak_mb'] = round(peak[name] / 2 ** 20, 1)
    line['score_tb_per_s'] = round(nbytes / (line['score_ms_median'] * 1e-3) / 1e12, 3)
    line['xentropy_tb_per_s'] = round(nbytes / (line['xentropy_ms_median'] * 1e-3) / 1e12, 3)
    line['score_over_xentropy'] = round(line['score_ms_median'] / line['xentropy_ms_median'], 3)
    line['torch_min_over_score_median'] = round(line['torch_ms_min'] / line['score_ms_median'], 2)
    line['score_median_below_torch_min'] = line['score_ms_median'] < line['torch_ms_min']
    emit(line, a.out)
    del logits, labels
    torch.cuda.empty_cache()
    if a.no_model:
        return

    from bench import MODELS
    from src.models.backpack import BackpackConfig, BackpackLMHeadModel
    from src.utils.perplexity import lm_loss_chunked
    from src.utils.scoring import evaluate_lm
    cfg = BackpackConfig(vocab_size=50257, n_positions=a.seq, scale_attn_by_inverse_layer_idx=True, use_flash_attn=True,
                         fused_bias_fc=True, fused_dense_gelu_dense=True, fused_dropout_add_ln=True, pad_vocab_size_multiple=8,
                         **MODELS['small'])
    torch.manual_seed(0)
    model = BackpackLMHeadModel(cfg, device=dev, dtype=torch.bfloat16).eval()
    ids = torch.randint(0, 50257, (a.batch, a.seq), device=dev)
    legs = {'evaluate_lm': lambda: evaluate_lm(model, [ids]), 'lm_loss_chunked': lambda: float(lm_loss_chunked(model, ids)[0])}
    ms, peak = alternate(legs, a.runs)
    tokens = a.batch * (a.seq - 1)
    line = {'bench': 'evaluate_lm', 'model': 'small', 'batch': a.batch, 'seq': a.seq, 'runs': a.runs}
    for name in legs:
        line[f'{name}_ms_runs'] = ms[name]
        line[f'{name}_tokens_per_s'] = round(tokens / (statistics.median(ms[name]) * 1e-3))
        line[f'{name}_peak_mb'] = round(peak[name] / 2 ** 20, 1)
    line['loss_evaluate_lm'] = evaluate_lm(model, [ids])['loss']
    line['loss_lm_loss_chunked'] = float(lm_loss_chunked(model, ids)[0])
    emit(line, a.out)


if __name__ == '__main__':
    main()
