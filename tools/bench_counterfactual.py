#!/usr/bin/env python3
"""Timing of VAR.abduct_noise / VAR.counterfactual on one MI355X, random-init weights (detinit seed 0), VAR-d16 256 x 256, B = 8, f32 and
bf16 (2 warm-up rounds, --iters (>= 5) timed rounds, median of HIP-event times; the variants alternate call by call inside a round, so they
see the same machine):
  (a) the calls: abduct_noise; counterfactual with K = 1 and with K = 4 target labels per image; and, on the same rows in the same process,
      VAR.autoregressive_infer_cfg_per_image_scored (one sampling walk and one decode), the comparator;
  (b) the kernels on the (B, l, V) of the largest scale: varhip_exp1_posterior_f32 and, on the same rows with the noise it wrote,
      varhip_cfg_sample_rows_f32 without filters (what the replay runs) and with top-k 900 / top-p 0.96.  --repeats repeats of --reps launches
      between one pair of events.  The posterior kernel's 3 * V * 4 bytes per row against the measured HBM copy rate
      profiles/best_of_pruned_bench.json uses (6.29 TB/s).

    python tools/bench_counterfactual.py [--precisions f32,bf16] [--iters 5] [--out profiles/counterfactual_bench.json]

Informational: no threshold is attached to any of these numbers.  Prints one JSON object (and writes it to --out)."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_compose import HERE, PNS, build_model, rounds_ms, summary  # noqa: E402

COPY_TBPS = 6.29            # the measured device-to-device copy rate of profiles/best_of_pruned_bench.json ("share_of_measured_copy_6p29TBps")


def kernel_bench(B: int, l: int, V: int, repeats: int, reps: int) -> dict:
    import torch
    from var_amd import hip
    g = torch.Generator(device='cuda').manual_seed(0)
    lg = torch.randn(2 * B * l, V, device='cuda', generator=g) * 3
    tt = torch.full((B,), 1.5, dtype=torch.float64, device='cuda')
    gt = torch.randint(0, V, (B * l,), device='cuda', generator=g)
    seeds = torch.arange(B, dtype=torch.int64, device='cuda') + 1000
    noise, logp = torch.empty(B * l, V, device='cuda'), torch.empty(B * l, device='cuda')
    flag = torch.empty(B * l, dtype=torch.int32, device='cuda')
    idx = torch.empty(B * l, dtype=torch.int64, device='cuda')
    k0, p0 = torch.zeros(B, dtype=torch.int32, device='cuda'), torch.zeros(B, dtype=torch.float64, device='cuda')
    k9, p9 = torch.full((B,), 900, dtype=torch.int32, device='cuda'), torch.full((B,), 0.96, dtype=torch.float64, device='cuda')
    fns = {'exp1_posterior': lambda: hip.call('exp1_posterior_f32', lg, tt, gt, l, seeds, B, l, V, 9, noise, logp, flag, l),
           'cfg_sample_rows no filter': lambda: hip.call('cfg_sample_rows_f32', lg, noise, idx, None, B, l, V, tt, k0, p0, V),
           'cfg_sample_rows top-k 900 top-p 0.96': lambda: hip.call('cfg_sample_rows_f32', lg, noise, idx, None, B, l, V, tt, k9, p9, 900)}
    out = {}
    for name, fn in fns.items():
        for _ in range(3):
            fn()
        us = []
        for _ in range(repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                fn()
            b.record(); torch.cuda.synchronize()
            us.append(a.elapsed_time(b) * 1e3 / reps)
        out[name] = dict(median_us=round(statistics.median(us), 2), min_us=round(min(us), 2), max_us=round(max(us), 2))
    out['flagged_rows'] = int(flag.sum())
    byts = 3.0 * V * 4 * B * l
    tbps = byts / (out['exp1_posterior']['median_us'] * 1e-6) / 1e12
    out['rows'], out['V'] = B * l, V
    out['exp1_posterior_bytes'] = byts
    out['exp1_posterior_TBps'] = round(tbps, 3)
    out['share_of_measured_copy_6p29TBps'] = round(tbps / COPY_TBPS, 3)
    out['posterior_over_sampler_no_filter'] = round(out['exp1_posterior']['median_us'] / out['cfg_sample_rows no filter']['median_us'], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--precisions', default='f32,bf16')
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--B', type=int, default=8)
    ap.add_argument('--out', default='')
    a = ap.parse_args()
    if a.iters < 5:
        ap.error('--iters must be at least 5')
    import torch
    vae, var = build_model(HERE)
    B = a.B
    lab = [(91 * b + 7) % 1000 for b in range(B)]
    dst1 = [(x + 500) % 1000 for x in lab]
    dst4 = [[(x + 100 * (k + 1)) % 1000 for k in range(4)] for x in lab]
    seeds, aseeds = [1000 + b for b in range(B)], [2000 + b for b in range(B)]
    res = dict(config=dict(model='d16', B=B, patch_nums=list(PNS), warmup=2, iters=a.iters, repeats=a.repeats, reps=a.reps, cfg=1.5,
                           weights='random init (detinit seed 0)', statistic='median of HIP-event times, variants alternating per round'))
    for prec in a.precisions.split(','):
        var.set_hip_precision(prec)
        tok = var.autoregressive_infer_cfg_per_image_scored(lab, seeds, cfg=1.5, decode=False).tokens
        fns = {'abduct_noise': lambda: var.abduct_noise(tok, lab, aseeds, cfg=1.5),
               'counterfactual K=1': lambda: var.counterfactual(tok, lab, dst1, aseeds, cfg=1.5),
               'counterfactual K=4': lambda: var.counterfactual(tok, lab, dst4, aseeds, cfg=1.5),
               'per_image_scored': lambda: var.autoregressive_infer_cfg_per_image_scored(lab, seeds, cfg=1.5),
               'per_image_scored no decode': lambda: var.autoregressive_infer_cfg_per_image_scored(lab, seeds, cfg=1.5, decode=False)}
        ms = {k: summary(v) for k, v in rounds_ms(fns, 2, a.iters).items()}
        walk, full = ms['per_image_scored no decode']['median_ms'], ms['per_image_scored']['median_ms']
        ms['abduct_over_walk_without_decode'] = round(ms['abduct_noise']['median_ms'] / walk, 3)
        ms['counterfactual_K1_over_two_walks_plus_decode'] = round(ms['counterfactual K=1']['median_ms'] / (walk + full), 3)
        ms['counterfactual_K4_over_K1'] = round(ms['counterfactual K=4']['median_ms'] / ms['counterfactual K=1']['median_ms'], 3)
        same = var.counterfactual(tok, lab, lab, aseeds, cfg=1.5, decode=False)
        ms['identity_holds'] = bool(torch.equal(same.tokens[:, 0], tok))
        ms['changed_share_K1'] = round(float(var.counterfactual(tok, lab, dst1, aseeds, cfg=1.5, decode=False).changed.float().mean()), 4)
        res[prec] = ms
    var.set_hip_precision('f32')
    res['kernels'] = kernel_bench(B, PNS[-1] ** 2, var.V, a.repeats, a.reps)
    txt = json.dumps(res)
    print(txt)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(txt + '\n')


if __name__ == '__main__':
    main()
