#!/usr/bin/env python3
"""Timing of direct logit attribution (VAR.logit_attribution) on one MI355X, random-init weights (detinit seed 0), d16, f32, N images of 256x256
given as tokens:

    attribution      var.logit_attribution(gt, labels)                          all 16 layers
    attribution_4    var.logit_attribution(gt, labels, layers=(3, 7, 11, 15))
    evaluate         var.evaluate(gt, labels)                                    the pass the call rides on
    torch            logit_attribution_torch on the same GPU                     hooks on the module stack, fp32

alternated in one process, and varhip_rowdot_seg_f64 alone on the widest scale's rows (HIP events around --reps launches, as GB/s of the bytes
it reads).  The recorded patch_effects sweep (profiles/patch_effects_bench.json, 288 rows for one image) is quoted for context: it answers the
total effect, this call the direct one.

    python tools/bench_logit_attribution.py [--images 8] [--iters 5] [--warmup 2] [--out profiles/logit_attribution_bench.json]

Prints one JSON object (and writes it to --out).  The FLOP-count expectation beside the measured ratio: per block and image the transformer
spends 2 * L * 12 C^2 in its GEMMs and the call adds one C x C GEMM, 2 * L * C^2, per selected block: (depth * 12 + D') / (depth * 12) of the
blocks' GEMM work, before the snapshot copies and the row dots, which move bytes and compute nothing."""
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
    ap.add_argument('--reps', type=int, default=20, help='launches of the kernel-alone rows')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    dev = torch.device('cuda', 0)
    from models import build_vae_var
    from var_amd.models.var import logit_attribution_torch
    pns = (1, 2, 3, 4, 5, 6, 8, 10, 13, 16)
    with contextlib.redirect_stdout(io.StringIO()):
        vae, var = build_vae_var(device=dev, patch_nums=pns, depth=16, ch=160)
    detinit.fill_module_device_(var, 16, 0, 'var.'); detinit.fill_module_device_(vae, 16, 0, 'vae.')
    var.eval(); vae.eval(); var.cond_drop_rate = 0.0
    N, L, V, C, D, H = a.images, var.L, var.V, var.C, var.depth, var.num_heads
    g = torch.Generator(device=dev).manual_seed(0)
    gt = torch.randint(0, V, (N, L), device=dev, generator=g)
    lab = torch.randint(0, 1000, (N,), device=dev, generator=g)
    four = (3, 7, 11, 15)
    ev = lambda: torch.cuda.Event(enable_timing=True)

    def timed(fn, reps=1):
        torch.cuda.synchronize()
        e0, e1 = ev(), ev()
        e0.record()
        for _ in range(reps):
            r = fn()
        e1.record()
        torch.cuda.synchronize()
        return r, e0.elapsed_time(e1) / reps

    res = dict(images=N, depth=D, L=L, V=V, iters=a.iters, warmup=a.warmup)
    with torch.inference_mode():
        routes = [('attribution', lambda: var.logit_attribution(gt, lab)), ('attribution_4', lambda: var.logit_attribution(gt, lab, layers=four)),
                  ('evaluate', lambda: var.evaluate(gt, lab)), ('torch', lambda: logit_attribution_torch(var, gt, lab, 'gt', None, None, N))]
        ms, last = {k: [] for k, _ in routes}, {}
        for _ in range(a.warmup):
            for _, fn in routes:
                timed(fn)
        for _ in range(a.iters):
            for k, fn in routes:
                last[k], t = timed(fn)
                ms[k].append(t)
        r = {k: dict(ms_median=statistics.median(ms[k]), ms_min=min(ms[k]), ms_max=max(ms[k])) for k, _ in routes}
        e = r['evaluate']
        e['spread'] = (e['ms_max'] - e['ms_min']) / e['ms_median']
        for k, n in (('attribution', D), ('attribution_4', 4)):
            r[k]['over_evaluate'] = r[k]['ms_median'] / e['ms_median']
            r[k]['gemm_flop_expectation'] = (D * 12 + n) / (D * 12)
        r['torch']['over_attribution'] = r['torch']['ms_median'] / r['attribution']['ms_median']
        r['completeness'] = last['attribution'].completeness()
        r['hip_vs_torch_max_abs'] = {k: float((getattr(last['attribution'], k).double() - last['torch'][k].double()).abs().max()) for k in ('attn', 'mlp', 'head', 'embed')}
        res['f32'] = r
        M = N * pns[-1] ** 2
        x, y = torch.randn(M, C, device=dev, generator=g), torch.randn(M, C, device=dev, generator=g)
        rows = []
        for nseg, ldb in ((1, C), (H, C), (1, 0)):
            out = torch.empty(M * nseg, dtype=torch.float64, device=dev)
            fn = lambda: hip.call('rowdot_seg_f64', x, C, y, ldb, M, C, nseg, out)
            timed(fn, 3)
            _, t = timed(fn, a.reps)
            nbytes = 4.0 * M * C * (2 if ldb else 1) + 8.0 * M * nseg
            rows.append(dict(M=M, C=C, nseg=nseg, ldb=ldb, us=1e3 * t, gbs=nbytes / (t * 1e-3) / 1e9))
        res['rowdot_seg'] = rows
    try:
        with open(os.path.join(ROOT, 'profiles', 'patch_effects_bench.json')) as f:
            res['patch_effects_recorded'] = json.load(f)
    except (OSError, ValueError):
        res['patch_effects_recorded'] = None
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(json.dumps(res, indent=1) + '\n')


if __name__ == '__main__':
    main()
