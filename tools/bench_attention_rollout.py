#!/usr/bin/env python3
"""Timing of VAR.attention_maps and VAR.attention_rollout on one MI355X, random-init weights (detinit seed 0), d16, N images of 256x256 given as
tokens, 8 targets, all 16 layers, f32:

    attention_maps      var.attention_maps(gt, labels, targets)                       (the teacher-forced pass + two launches per layer)
    attention_rollout   var.attention_rollout(gt, labels, targets)                    (the same pass + two launches per layer, last to first)
    attention_profile   var.attention_profile(gt, labels)                             (the pass they ride on, with its own reductions)
    maps_torch          attention_maps_torch on the same GPU                          (per image and layer softmax(QK^T + mask) in float64)
    rollout_torch       attention_rollout_torch on the same GPU

alternated in one process, and the two kernels alone at Lq = 680 (rows = N, H = 16, T = 8) with HIP events around `reps` launches.

    python tools/bench_attention_rollout.py [--images 8] [--iters 5] [--warmup 2] [--out profiles/attention_rollout_bench.json]

Prints one JSON object (and writes it to --out): median / min / max ms per call of every route, the ratios to the plain pass and to the torch
routes, the largest difference between the HIP and the torch routes, and the per-launch times of the two kernels."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=8)
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--reps', type=int, default=20, help='launches of each kernel in the kernel-alone table')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    dev = torch.device('cuda', 0)
    from models import build_vae_var
    from var_amd.models.var import attention_maps_torch, attention_rollout_torch
    pns = (1, 2, 3, 4, 5, 6, 8, 10, 13, 16)
    with contextlib.redirect_stdout(io.StringIO()):
        vae, var = build_vae_var(device=dev, patch_nums=pns, depth=16, ch=160)
    detinit.fill_module_device_(var, 16, 0, 'var.'); detinit.fill_module_device_(vae, 16, 0, 'vae.')
    var.eval(); vae.eval(); var.cond_drop_rate = 0.0
    N, L, S, H, D = a.images, var.L, len(pns), var.num_heads, var.depth
    g = torch.Generator(device=dev).manual_seed(0)
    gt = torch.randint(0, var.V, (N, L), device=dev, generator=g)
    lab = torch.randint(0, 1000, (N,), device=dev, generator=g)
    layers = tuple(range(D))
    targets = (0, 3, 20, 60, 120, 300, 500, 679)
    T = len(targets)
    ev = lambda: torch.cuda.Event(enable_timing=True)

    def timed(fn, n=1):
        torch.cuda.synchronize()
        e0, e1 = ev(), ev()
        e0.record()
        for _ in range(n):
            r = fn()
        e1.record()
        torch.cuda.synchronize()
        return r, e0.elapsed_time(e1) / n

    routes = [('attention_maps', lambda: var.attention_maps(gt, lab, targets, max_rows=N).rows),
              ('attention_rollout', lambda: var.attention_rollout(gt, lab, targets, max_rows=N).flow),
              ('attention_profile', lambda: var.attention_profile(gt, lab).share_q),
              ('maps_torch', lambda: attention_maps_torch(var, gt, lab, targets, layers)[0]),
              ('rollout_torch', lambda: attention_rollout_torch(var, gt, lab, targets, layers, 0.5)[0])]
    res = dict(images=N, depth=D, heads=H, L=L, scales=S, targets=T, iters=a.iters, warmup=a.warmup, softmax_mb_per_image=D * H * L * L * 4 / 1e6,
               stash_mb_per_image=D * L * var.C * 4 / 1e6)
    with torch.inference_mode():
        ms, last = {k: [] for k, _ in routes}, {}
        for _ in range(a.warmup):
            for _, fn in routes:
                timed(fn)
        for _ in range(a.iters):
            for k, fn in routes:
                last[k], t = timed(fn)
                ms[k].append(t)
        for k, _ in routes:
            res[k] = dict(ms_median=statistics.median(ms[k]), ms_min=min(ms[k]), ms_max=max(ms[k]))
        for k, tw in (('attention_maps', 'maps_torch'), ('attention_rollout', 'rollout_torch')):
            res[k]['over_attention_profile'] = res[k]['ms_median'] / res['attention_profile']['ms_median']
            res[tw]['over_hip_route'] = res[tw]['ms_median'] / res[k]['ms_median']
            res[k]['max_abs_vs_torch'] = float((last[k] - last[tw]).abs().max())
        # the two kernels alone at Lq = L
        q = torch.randn(N, L, H * 64, device=dev, generator=g)
        kc = torch.nn.functional.normalize(torch.randn(N, H, L + 8, 64, device=dev, generator=g), dim=-1)
        m, rinv = torch.empty(N, H, L, device=dev), torch.empty(N, H, L, device=dev)
        nanq = torch.zeros(N, H, dtype=torch.int32, device=dev)
        r = torch.rand(N, T, L, device=dev, generator=g)
        out1, out0 = torch.empty(N, H, T, L, device=dev), torch.empty(N, T, L, device=dev)
        ends = torch.tensor([e for _, e in var.begin_ends], dtype=torch.int32)
        kern = dict(Lq=L, rows=N, heads=H, targets=T, reps=a.reps)
        for name, fn in (('rowstats_us', lambda: hip.call('attn_rowstats_f32', q, kc, N, L, H, L + 8, ends, S, m, rinv, nanq)),
                         ('flow_per_head_us', lambda: hip.call('attn_flow_f32', q, kc, m, rinv, r, out1, N, L, H, L + 8, ends, S, T, 1, 0.5)),
                         ('flow_mean_us', lambda: hip.call('attn_flow_f32', q, kc, m, rinv, r, out0, N, L, H, L + 8, ends, S, T, 0, 0.5))):
            timed(fn, 3)
            kern[name] = 1e3 * timed(fn, a.reps)[1]
        res['kernels_alone'] = kern
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(json.dumps(res, indent=1) + '\n')


if __name__ == '__main__':
    main()
