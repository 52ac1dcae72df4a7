#!/usr/bin/env python3
"""Timing of VAR.sample_controlled on one MI355X, random-init weights (detinit seed 0), VAR-d16 256 x 256, cfg 1.5, top-k 900, top-p 0.96, at
B = 8 and B = 64 (2 warm-up rounds, --iters (>= 5) timed rounds, median of HIP-event times; the variants of a comparison alternate call by
call inside a round, so they see the same machine):
  (a) sample_controlled with default controls, and with every control active (temperature, min-p, a (B, V) logit bias with bans, per-scale
      schedules of all knobs), against VAR.autoregressive_infer_cfg_per_image_scored, whose code path this change does not touch;
  (b) the sampler kernels on the (B, l, V) of the last scale: varhip_cfg_sample_rows_f32, varhip_mix_sample_rows_f32 at G = 2 (the two
      instantiations of the shared body that existed before) and varhip_ctl_sample_rows_f32 with null and with active controls.  --repeats
      (default 5) repeats, each --reps launches between one pair of events; per launch: median, min and max over the repeats.  The same
      command on a checkout of the parent commit (--kernels-only; the controlled entry is skipped where the library has none) gives the
      numbers to compare: this commit's median must not exceed the parent's slowest repeat by more than the parent's max - min.

    python tools/bench_controlled.py [--precisions f32] [--iters 5] [--Bs 8,64] [--out profiles/controlled_bench.json]
    python tools/bench_controlled.py --kernels-only

Informational: no threshold is attached to any of these numbers.  Prints one JSON object (and writes it to --out)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_compose import HERE, KW, PNS, build_model, rounds_ms, summary  # noqa: E402

S = len(PNS)


def active_controls(B: int, V: int) -> dict:
    """every stage of the sampler running: per-scale schedules of the five knobs and one bias row per image with a third of the codes banned"""
    rng = np.random.default_rng(0)
    bias = rng.standard_normal((B, V)).astype(np.float32)
    bias[:, rng.permutation(V)[:V // 3]] = -np.inf
    col = lambda lo, hi: np.linspace(lo, hi, S)[:, None]
    return dict(cfg=col(1.0, 3.0), top_k=np.linspace(1200, 600, S).astype(np.int64)[:, None], top_p=col(0.99, 0.9), temperature=col(1.3, 0.8),
                min_p=col(0.02, 0.005), logit_bias=bias, cfg_ramp=False)


def kernel_bench(B: int, l: int, V: int, repeats: int, reps: int) -> dict:
    import torch
    from var_amd import hip
    g = torch.Generator(device='cuda').manual_seed(0)
    noise = torch.empty(B * l, V, device='cuda').exponential_(1, generator=g)
    idx = torch.empty(B * l, dtype=torch.int64, device='cuda')
    masked = torch.empty(B * l, V, device='cuda')
    lg = torch.randn(2 * B * l, V, device='cuda', generator=g) * 3
    tk = torch.full((B,), 900, dtype=torch.int32, device='cuda')
    tp = torch.full((B,), 0.96, dtype=torch.float64, device='cuda')
    tt = torch.full((B,), 1.5, dtype=torch.float64, device='cuda')
    coef = torch.tensor([[2.5, 1.5]] * B, dtype=torch.float32, device='cuda')
    one, zero = torch.ones(B, device='cuda'), torch.zeros(B, device='cuda')
    tau, mp = torch.full((B,), 0.8, device='cuda'), torch.full((B,), 0.01, device='cuda')
    bias = torch.randn(B, V, device='cuda', generator=g)
    brow = torch.arange(B, dtype=torch.int32, device='cuda')
    fns = {'cfg_sample_rows': lambda: hip.call('cfg_sample_rows_f32', lg, noise, idx, masked, B, l, V, tt, tk, tp, 900),
           'mix_sample_rows G=2': lambda: hip.call('mix_sample_rows_f32', lg, noise, idx, masked, None, B, l, V, 2, coef, tk, tp, 900)}
    if 'ctl_sample_rows_f32' in hip.lib().fn:
        fns['ctl_sample_rows null controls'] = lambda: hip.call('ctl_sample_rows_f32', lg, noise, idx, masked, B, l, V, tt, tk, tp, one, zero, None, None, 0, 0, 900)
        fns['ctl_sample_rows tau, min_p, bias'] = lambda: hip.call('ctl_sample_rows_f32', lg, noise, idx, masked, B, l, V, tt, tk, tp, tau, mp, bias, brow, B, V, 900)
    ms = rounds_ms({k: (lambda f=f: [f() for _ in range(reps)]) for k, f in fns.items()}, 2, repeats)
    out = {}
    for k in fns:
        per = [x / reps * 1e3 for x in ms[k]]
        out[k] = dict(us_per_launch=round(statistics.median(per), 2), min_us=round(min(per), 2), max_us=round(max(per), 2), repeats=[round(x, 2) for x in per])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--precisions', default='f32')
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--Bs', default='8,64')
    ap.add_argument('--kernels-only', action='store_true')
    ap.add_argument('--out', default='')
    a = ap.parse_args()
    if a.iters < 5 or a.repeats < 5:
        ap.error('--iters and --repeats must be at least 5')
    Bs = [int(x) for x in a.Bs.split(',')]
    res = dict(model='VAR-d16 256x256, detinit seed 0', iters=a.iters, **KW)
    if a.kernels_only:
        sys.path.insert(0, HERE)
        V = 4096
    else:
        import torch
        vae, var = build_model(HERE)
        V = var.V
        calls = {}
        for prec in a.precisions.split(','):
            var.set_hip_precision(prec)
            for B in Bs:
                lab, seeds = [(91 * b + 7) % 1000 for b in range(B)], [1000 + b for b in range(B)]
                act = active_controls(B, V)
                fns = {'per_image_scored': lambda: var.autoregressive_infer_cfg_per_image_scored(lab, seeds, **KW),
                       'controlled, default controls': lambda: var.sample_controlled(lab, seeds, **KW),
                       'controlled, all controls active': lambda: var.sample_controlled(lab, seeds, **act),
                       'per_image_scored (again)': lambda: var.autoregressive_infer_cfg_per_image_scored(lab, seeds, **KW)}
                r = {k: summary(v) for k, v in rounds_ms(fns, 2, a.iters).items()}
                ref, rec = fns['per_image_scored'](), fns['controlled, default controls']()
                r['default controls equal the per-image scored call (tokens, images)'] = bool(torch.equal(ref.tokens, rec.tokens) and torch.equal(ref.images, rec.images))
                r['ratio to per_image_scored'] = {k: round(v['median_ms'] / r['per_image_scored']['median_ms'], 4) for k, v in r.items() if isinstance(v, dict)}
                calls[f'{prec} B={B}'] = r
        var.set_hip_precision('f32')
        res['a_calls'] = calls
    res['b_kernels'] = {f'B={B}': dict(l=PNS[-1] ** 2, V=V, top_k=900, top_p=0.96, reps=a.reps, **kernel_bench(B, PNS[-1] ** 2, V, a.repeats, a.reps)) for B in Bs}
    text = json.dumps(res, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)) or '.', exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
