#!/usr/bin/env python3
"""Timing of the distance-probability profile (fork var_analysis.py:352-425 + :694-732) on one MI355X, random-init weights (detinit seed 0),
d16, N images of 256x256 given as tokens, K candidate classes, edges = linspace(0, 30, 100), in f32 with cfg 0 and in bf16 with cfg 1.5:

    distance_profile   var.distance_profile(gt, classes, edges, cfg=cfg, min_prob=1e-10)
    log_likelihood     var.token_log_likelihood(gt, classes, cfg=cfg)           (the yardstick: the bar is at most 10 % over it)
    expected_distance  var.token_scores(gt, classes, 'expected_distance', cfg=cfg)   (reads the same bytes)
    old                the fork's route per image: logits = var(label, x) (+ the unconditional forward and the guided combine), torch softmax,
                       the gathered table rows, then torch.bucketize + index_add_ of counts and probabilities per scale (every pair, no subsample)

all in one process, alternated, the old one on a stream of its own (it keeps its own workspace).

    python tools/bench_distance_profile.py [--images 8] [--classes 10] [--iters 5] [--warmup 2] [--out profiles/distance_profile_bench.json]

Prints one JSON object (and writes it to --out): per configuration the median, min and max ms per call of every route (HIP events), the rise of
torch.cuda.max_memory_allocated over a call, the ratio to log_likelihood, and the scoring kernels' own time per call from the library's timing
table (family 'sampler') for distance_profile and expected_distance with their bytes/s against the 8 TB/s HBM peak."""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from var_amd import detinit, hip      # noqa: E402

HBM_PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=8)
    ap.add_argument('--classes', type=int, default=10)
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    dev = torch.device('cuda', 0)
    from models import build_vae_var
    pns = (1, 2, 3, 4, 5, 6, 8, 10, 13, 16)
    with contextlib.redirect_stdout(io.StringIO()):
        vae, var = build_vae_var(device=dev, patch_nums=pns, depth=16, ch=160)
    detinit.fill_module_device_(var, 16, 0, 'var.'); detinit.fill_module_device_(vae, 16, 0, 'vae.')
    var.eval(); vae.eval(); var.cond_drop_rate = 0.0
    N, K, V, L, S = a.images, a.classes, var.V, var.L, len(pns)
    g = torch.Generator(device=dev).manual_seed(0)
    gt = torch.randint(0, V, (N, L), device=dev, generator=g)
    classes = torch.randperm(1000, device=dev, generator=g)[:K]
    edges = torch.linspace(0, 30, 100)
    edges_d = edges.to(dev)
    B = edges.numel() - 1
    min_prob = 1e-10
    ratio = torch.tensor([si / (S - 1) for si, pn in enumerate(pns) for _ in range(pn * pn)], device=dev)
    ev = lambda: torch.cuda.Event(enable_timing=True)
    side = torch.cuda.Stream()

    def old_route(cfg):
        dist = var.engine().code_distance_table()
        x = vae.quantize.idxBl_to_var_input([gt[:, b:e] for b, e in var.begin_ends])
        t = cfg * ratio.view(1, -1, 1)
        count = torch.zeros(N, K, S, B, dtype=torch.int64, device=dev)
        mass = torch.zeros(N, K, S, B, dtype=torch.float64, device=dev)
        koff = torch.arange(K, device=dev).view(K, 1, 1) * B
        for i in range(N):
            z = var(classes, x[i:i + 1].expand(K, -1, -1).contiguous())
            if cfg > 0:
                z = (1 + t) * z - t * var(torch.tensor([var.num_classes], device=dev), x[i:i + 1].contiguous())
            p = torch.softmax(z, dim=-1)                                  # (K, L, V)
            d = dist[gt[i]].unsqueeze(0).expand(K, L, V).contiguous()     # (K, L, V)
            b = torch.bucketize(d, edges_d, right=True) - 1
            ok = (b >= 0) & (b < B) & (p > min_prob)
            for si, (t0, t1) in enumerate(var.begin_ends):
                sel = ok[:, t0:t1]
                cell = (koff + b[:, t0:t1].clamp(0, B - 1))[sel]
                count[i, :, si] = torch.zeros(K * B, dtype=torch.int64, device=dev).index_add_(0, cell, torch.ones_like(cell)).view(K, B)
                mass[i, :, si] = torch.zeros(K * B, dtype=torch.float64, device=dev).index_add_(0, cell, p[:, t0:t1][sel].double()).view(K, B)
        return count, mass

    def timed(fn, stream):
        with torch.cuda.stream(stream):
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            e0, e1 = ev(), ev()
            e0.record()
            r = fn()
            e1.record()
            torch.cuda.synchronize()
            return r, e0.elapsed_time(e1), torch.cuda.max_memory_allocated() - base

    def kernel_time(fn):
        hip.timing_reset(); hip.timing_enable(True, ['sampler'])
        fn()
        torch.cuda.synchronize()
        tt = hip.timing_read()['sampler']
        hip.timing_enable(False)
        rate = tt['bytes'] / (tt['ms'] * 1e-3) if tt['ms'] > 0 else None
        return dict(ms_per_call=tt['ms'], launches=tt['launches'], bytes=tt['bytes'], TBps=rate / 1e12 if rate else None,
                    frac_of_hbm_peak=rate / HBM_PEAK if rate else None)

    res = dict(images=N, classes=K, depth=16, L=L, V=V, bins=B, min_prob=min_prob, iters=a.iters, warmup=a.warmup,
               full_logits_mb_per_image=K * L * V * 4 / 1e6)
    with torch.inference_mode():
        for dtype, cfg in (('f32', 0.0), ('bf16', 1.5)):
            var.set_hip_precision(dtype)
            main_s = torch.cuda.current_stream()
            routes = [('distance_profile', lambda: var.distance_profile(gt, classes, edges, cfg=cfg, min_prob=min_prob), main_s),
                      ('log_likelihood', lambda: var.token_log_likelihood(gt, classes, cfg=cfg), main_s),
                      ('expected_distance', lambda: var.token_scores(gt, classes, 'expected_distance', cfg=cfg), main_s),
                      ('old', lambda: old_route(cfg), side)]
            for _ in range(a.warmup):
                for _, fn, st in routes:
                    timed(fn, st)
            ms, peak, last = {k: [] for k, _, _ in routes}, {k: 0 for k, _, _ in routes}, {}
            for _ in range(a.iters):                                                                         # alternated
                for k, fn, st in routes:
                    last[k], t_ms, pk = timed(fn, st)
                    ms[k].append(t_ms); peak[k] = max(peak[k], pk)
            d = {}
            for k, _, _ in routes:
                med = statistics.median(ms[k])
                d[k] = dict(ms_median=med, ms_min=min(ms[k]), ms_max=max(ms[k]), peak_alloc_mb=peak[k] / 1e6)
            for k in ('distance_profile', 'expected_distance', 'old'):
                d[k]['over_log_likelihood'] = d[k]['ms_median'] / d['log_likelihood']['ms_median']
            new, (oc, om) = last['distance_profile'], last['old']
            d['old_vs_new'] = dict(speedup_at_median=d['old']['ms_median'] / d['distance_profile']['ms_median'],
                                   counts_equal=bool(torch.equal(new.count_NKSB, oc)),
                                   count_cells_differing=int((new.count_NKSB != oc).sum()),
                                   max_rel_mass_delta=float(((new.mass_NKSB - om).abs() / om.clamp_min(1e-300)).max()))
            d['kernel'] = dict(distance_profile=kernel_time(routes[0][1]), expected_distance=kernel_time(routes[2][1]))
            res[f'{dtype}_cfg{cfg:g}'] = d
        var.set_hip_precision('f32')
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(json.dumps(res, indent=1) + '\n')


if __name__ == '__main__':
    main()
