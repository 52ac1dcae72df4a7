#!/usr/bin/env python3
"""Timing of the logit lens (VAR.logit_lens) on one MI355X, random-init weights (detinit seed 0), d16, N images of 256x256 given as tokens, in
f32 and bf16:

    logit_lens      var.logit_lens(gt, labels)                       all 16 layers: the teacher-forced pass + per scale 15 more head GEMMs and 16 reductions
    logit_lens_4    var.logit_lens(gt, labels, layers=(3, 7, 11, 15))
    evaluate        var.evaluate(gt, labels)                         the pass the call rides on, with its one head and varhip_token_eval_f32
    torch           logit_lens_torch on the same GPU (f32 only)      forward hooks, get_logits per hook, float64 log-softmaxes

alternated in one process, and per scale varhip_token_lens_f32 alone next to varhip_token_eval_f32 on rows of the call's shape (HIP events around
--reps launches; the lens kernel reads two rows per token, token_eval one: both as GB/s of the bytes each reads).

    python tools/bench_logit_lens.py [--images 8] [--iters 5] [--warmup 2] [--out profiles/logit_lens_bench.json]

Prints one JSON object (and writes it to --out).  The FLOP-count expectation beside the measured ratio: per block and image the transformer spends
2 * L * 12 C^2 = 17 GF in its GEMMs, one head GEMM 2 * L * C * V = 5.7 GF, so logit_lens with D' layers should cost about
(depth * 17 + D' * 5.7) / (depth * 17 + 5.7) of evaluate (the last selected layer's head is evaluate's own when it is the model's last block)."""
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
    ap.add_argument('--reps', type=int, default=20, help='launches per scale of the kernel-alone table')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    dev = torch.device('cuda', 0)
    from models import build_vae_var
    from var_amd.models.var import LogitLens, logit_lens_torch
    pns = (1, 2, 3, 4, 5, 6, 8, 10, 13, 16)
    with contextlib.redirect_stdout(io.StringIO()):
        vae, var = build_vae_var(device=dev, patch_nums=pns, depth=16, ch=160)
    detinit.fill_module_device_(var, 16, 0, 'var.'); detinit.fill_module_device_(vae, 16, 0, 'vae.')
    var.eval(); vae.eval(); var.cond_drop_rate = 0.0
    N, L, V, C, D = a.images, var.L, var.V, var.C, var.depth
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

    block_gf, head_gf = 2 * L * 12 * C * C / 1e9, 2 * L * C * V / 1e9      # (the four GEMMs of a block; attention comes on top)
    expect = lambda n: (D * block_gf + n * head_gf) / (D * block_gf + head_gf)
    res = dict(images=N, depth=D, L=L, V=V, iters=a.iters, warmup=a.warmup, block_gflop_per_image=block_gf, head_gflop_per_image=head_gf,
               per_layer_logits_mb=N * L * V * 4 / 1e6)
    with torch.inference_mode():
        for prec in ('f32', 'bf16'):
            var.set_hip_precision(prec)
            routes = [('logit_lens', lambda: var.logit_lens(gt, lab)), ('logit_lens_4', lambda: var.logit_lens(gt, lab, layers=four)),
                      ('evaluate', lambda: var.evaluate(gt, lab))]
            if prec == 'f32':
                routes.append(('torch', lambda: LogitLens(tuple(range(D)), *logit_lens_torch(var, gt, lab, tuple(range(D)), N), pns)))
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
            r['evaluate']['spread'] = (e['ms_max'] - e['ms_min']) / e['ms_median']
            for k, n in (('logit_lens', D), ('logit_lens_4', 4)):
                r[k]['over_evaluate'] = r[k]['ms_median'] / e['ms_median']
                r[k]['flop_expectation'] = expect(n)
            if prec == 'f32':
                r['torch']['over_logit_lens'] = r['torch']['ms_median'] / r['logit_lens']['ms_median']
                r['hip_vs_torch_max_abs'] = {k: float((getattr(last['logit_lens'], k) - getattr(last['torch'], k)).abs().max()) for k in ('nll', 'entropy', 'kl')}
            res[prec] = r
        var.set_hip_precision('f32')
        # per scale, the kernel alone next to varhip_token_eval_f32: rows of the call's shape
        table = []
        for pn in pns:
            l = pn * pn
            z, zf = torch.randn(N * l, V, device=dev, generator=g) * 4, torch.randn(N * l, V, device=dev, generator=g) * 4
            tok = torch.randint(0, V, (N, l), device=dev, generator=g)
            f = lambda dt=torch.float32: torch.empty(N, l, dtype=dt, device=dev)
            o = [f(), f(), f(), f(torch.int64), f(torch.int32)]
            lens = lambda: hip.call('token_lens_f32', z, zf, tok, l, N, l, V, *o, l)
            evl = lambda: hip.call('token_eval_f32', z, tok, l, N, l, V, o[0], o[1], o[3], o[4], l)
            row = dict(l=l, rows=N * l)
            for name, fn, nbytes in (('token_lens', lens, 8.0 * V * N * l), ('token_eval', evl, 4.0 * V * N * l)):
                timed(fn, 3)
                _, t = timed(fn, a.reps)
                row[name + '_us'] = 1e3 * t
                row[name + '_gbs'] = nbytes / (t * 1e-3) / 1e9
            table.append(row)
        res['per_scale'] = table
        res['per_scale_sum_us'] = dict(token_lens=sum(r['token_lens_us'] for r in table), token_eval=sum(r['token_eval_us'] for r in table))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(json.dumps(res, indent=1) + '\n')


if __name__ == '__main__':
    main()
