#!/usr/bin/env python3
"""Timing of head / MLP ablation and activation patching (VAR.patch_effects) on one MI355X, random-init weights (detinit seed 0), d16, f32, one
image of 256x256 given as tokens, the full default sweep (256 heads + 16 attention layers + 16 MLPs = 288 sites, 289 rows with the clean one):

    patch_effects   var.patch_effects(gt, label, mode=...)           in each mode ('donor' adds the donor row to every pass), max_rows 64
    plain_pass      var.token_log_likelihood(gt, 289 labels)         the same number of rows through the same passes with no intervention
    torch           patch_effects_torch on the same GPU ('mean')     the hook route: one masked forward per site

alternated in one process, and varhip_act_patch_f32 alone at the last scale's shapes of a 64-row pass (att: [64 * 256][1024], one head of every
row but the clean one, in each mode; hid: [64 * 256][4096], the whole width of one row), HIP events around --reps launches, with the bytes each
moves (zero: the stores; mean and copy: one load and one store per element) and the bandwidth that makes.

    python tools/bench_patch_effects.py [--iters 5] [--warmup 2] [--out profiles/patch_effects_bench.json]

Prints one JSON object (and writes it to --out).  The design expectation beside the measured ratio: a patched block adds two short launches to
seven, and only the blocks that hold a site of the pass are patched, so the sweep should stay close to the plain pass of equal rows."""
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
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--reps', type=int, default=50, help='launches of the kernel-alone table')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    dev = torch.device('cuda', 0)
    from models import build_vae_var
    from var_amd.models import args as A
    from var_amd.models.var import patch_effects_torch
    pns = (1, 2, 3, 4, 5, 6, 8, 10, 13, 16)
    with contextlib.redirect_stdout(io.StringIO()):
        vae, var = build_vae_var(device=dev, patch_nums=pns, depth=16, ch=160)
    detinit.fill_module_device_(var, 16, 0, 'var.'); detinit.fill_module_device_(vae, 16, 0, 'vae.')
    var.eval(); vae.eval(); var.cond_drop_rate = 0.0
    L, V, C, D, H = var.L, var.V, var.C, var.depth, var.num_heads
    hidden = var.blocks[0].ffn.fc1.weight.shape[0]
    g = torch.Generator(device=dev).manual_seed(0)
    gt = torch.randint(0, V, (1, L), device=dev, generator=g)
    lab = torch.tensor([207], device=dev)
    sites = A.patch_sites(None, D, H)
    cols = A.patch_columns(sites, C, hidden)
    rows = len(sites) + 1
    many = torch.randint(0, 1000, (1, rows), device=dev, generator=g)
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

    res = dict(images=1, depth=D, heads=H, L=L, V=V, sites=len(sites), rows=rows, max_rows=64, iters=a.iters, warmup=a.warmup)
    with torch.inference_mode():
        routes = [('patch_effects_' + m, (lambda m=m: var.patch_effects(gt, lab, mode=m, donor_label=1000 if m == 'donor' else None))) for m in A.PATCH_MODES]
        routes.append(('plain_pass', lambda: var.token_log_likelihood(gt, many)))
        routes.append(('torch', lambda: patch_effects_torch(var, gt, lab, cols, 'mean', None, tuple(range(len(pns))))))
        ms, last = {k: [] for k, _ in routes}, {}
        for _ in range(a.warmup):
            for _, fn in routes:
                timed(fn)
        for _ in range(a.iters):
            for k, fn in routes:
                last[k], t = timed(fn)
                ms[k].append(t)
        r = {k: dict(ms_median=statistics.median(ms[k]), ms_min=min(ms[k]), ms_max=max(ms[k])) for k, _ in routes}
        p = r['plain_pass']
        p['spread'] = (p['ms_max'] - p['ms_min']) / p['ms_median']
        for m in A.PATCH_MODES:
            r['patch_effects_' + m]['over_plain_pass'] = r['patch_effects_' + m]['ms_median'] / p['ms_median']
        r['torch']['over_patch_effects_mean'] = r['torch']['ms_median'] / r['patch_effects_mean']['ms_median']
        hipr, tor = last['patch_effects_mean'], last['torch']
        r['hip_vs_torch_max_abs'] = {k: float((getattr(hipr, k).double() - t.double()).abs().max()) for k, t in zip(('nll', 'entropy', 'kl'), tor)}
        res['calls'] = r
        # the kernel alone at the last scale of a 64-row pass
        R, l = 64, pns[-1] ** 2
        att, hid = torch.randn(R * l, C, device=dev, generator=g), torch.randn(R * l, hidden, device=dev, generator=g)
        table = []
        for name, act, width, dirs, per_elem in (
                ('att zero: a head of 63 rows', att, C, [(r_, 64 * (r_ % H), 64 * (r_ % H) + 64, -1) for r_ in range(1, R)], 4),
                ('att mean: a head of 63 rows', att, C, [(r_, 64 * (r_ % H), 64 * (r_ % H) + 64, -2) for r_ in range(1, R)], 8),
                ('att copy: a head of 62 rows', att, C, [(r_, 64 * (r_ % H), 64 * (r_ % H) + 64, 0) for r_ in range(2, R)], 8),
                ('att zero: all heads of a row', att, C, [(1, 0, C, -1)], 4), ('att mean: all heads of a row', att, C, [(1, 0, C, -2)], 8),
                ('hid zero: a row', hid, hidden, [(1, 0, hidden, -1)], 4), ('hid mean: a row', hid, hidden, [(1, 0, hidden, -2)], 8),
                ('hid copy: a row', hid, hidden, [(1, 0, hidden, 0)], 8)):
            d = torch.tensor(dirs, dtype=torch.int32).to(dev)
            fn = lambda: hip.call('act_patch_f32', act, width, R, l, width, d, len(dirs))
            timed(fn, 3)
            _, t = timed(fn, a.reps)
            nbytes = sum((c1 - c0) * l * per_elem for _, c0, c1, _ in dirs)
            table.append(dict(case=name, directives=len(dirs), l=l, bytes=nbytes, us=1e3 * t, gbs=nbytes / (t * 1e-3) / 1e9))
        res['kernel_alone'] = table
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(json.dumps(res, indent=1) + '\n')


if __name__ == '__main__':
    main()
