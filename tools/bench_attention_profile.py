#!/usr/bin/env python3
"""Timing of the attention profile (VAR.attention_profile) on one MI355X, random-init weights (detinit seed 0), d16, N images of 256x256 given as
tokens, all 16 layers, f32:

    attention_profile  var.attention_profile(gt, labels)                             (the teacher-forced pass + one reduction per layer and scale)
    log_likelihood     var.token_log_likelihood(gt, labels.view(N, 1))               (K = 1, cfg 0: the teacher-forced pass the call rides on, with its head)
    torch              attention_profile_torch on the same GPU                       (per layer softmax(QK^T + mask) in float64, then segment sums)

alternated in one process, and per scale the kernel alone next to k_attn_cached on operands of the call's shape (rows = N, H = 16), both from the
library's timing table (families 'attn_profile' and 'attn').

    python tools/bench_attention_profile.py [--images 8] [--iters 5] [--warmup 2] [--out profiles/attention_profile_bench.json]

Prints one JSON object (and writes it to --out): median / min / max ms per call of every route (HIP events), the ratios, the largest per-share
difference between the HIP and the torch route, the kernel's total time inside one call, and the per-scale table."""
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
    from var_amd.models.var import SHARE_ONE, AttentionProfile, attention_profile_torch
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
    ev = lambda: torch.cuda.Event(enable_timing=True)

    def timed(fn):
        torch.cuda.synchronize()
        e0, e1 = ev(), ev()
        e0.record()
        r = fn()
        e1.record()
        torch.cuda.synchronize()
        return r, e0.elapsed_time(e1)

    routes = [('attention_profile', lambda: var.attention_profile(gt, lab)),
              ('log_likelihood', lambda: var.token_log_likelihood(gt, lab.view(N, 1))),
              ('torch', lambda: AttentionProfile(*attention_profile_torch(var, gt, lab, 1, layers), pns, 1, layers))]
    res = dict(images=N, depth=D, heads=H, L=L, scales=S, iters=a.iters, warmup=a.warmup, softmax_mb_per_image=D * H * L * L * 4 / 1e6)
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
        res['attention_profile']['over_log_likelihood'] = res['attention_profile']['ms_median'] / res['log_likelihood']['ms_median']
        res['torch']['over_attention_profile'] = res['torch']['ms_median'] / res['attention_profile']['ms_median']
        res['hip_vs_torch_max_abs_share'] = float((last['attention_profile'].scale_matrix() - last['torch'].scale_matrix()).abs().max())
        # the kernels inside one call
        hip.timing_reset(); hip.timing_enable(True, ['attn_profile', 'attn'])
        routes[0][1]()
        torch.cuda.synchronize()
        tt = hip.timing_read()
        hip.timing_enable(False)
        res['inside_one_call'] = {k: dict(ms=tt[k]['ms'], launches=tt[k]['launches']) for k in ('attn_profile', 'attn')}
        # per scale, the kernel alone next to k_attn_cached: operands of the call's shape
        table = []
        ends_all = [e for _, e in var.begin_ends]
        for si, pn in enumerate(pns):
            l, curL = pn * pn, ends_all[si]
            q = torch.randn(N, l, H * 64, device=dev, generator=g)
            kc = torch.nn.functional.normalize(torch.randn(N, H, L, 64, device=dev, generator=g), dim=-1)
            vc = torch.randn(N, H, L, 64, device=dev, generator=g)
            out = torch.empty(N, l, H * 64, device=dev)
            share = torch.zeros(N, H, si + 2, dtype=torch.int64, device=dev)
            nanq = torch.zeros(N, H, dtype=torch.int32, device=dev)
            ends = torch.tensor(ends_all[:si + 1], dtype=torch.int32)
            row = dict(scale=si, l=l, curL=curL)
            for fam, fn in (('attn_profile', lambda: hip.call('attn_profile_f32', q, kc, N, l, H, curL, L, ends, si + 1, pn, 1, share, H * (si + 2), si + 2,
                                                               nanq, None, 0, 0)),
                            ('attn', lambda: hip.call('attn_cached_f32', q, kc, vc, out, N, l, H, curL, L))):
                for _ in range(3):
                    fn()
                torch.cuda.synchronize()
                hip.timing_reset(); hip.timing_enable(True, [fam])
                for _ in range(a.reps):
                    fn()
                torch.cuda.synchronize()
                t = hip.timing_read()[fam]
                hip.timing_enable(False)
                row[fam + '_us'] = 1e3 * t['ms'] / max(t['launches'], 1)
            row['ratio'] = row['attn_profile_us'] / row['attn_us']
            table.append(row)
        res['per_scale'] = table
        res['per_scale_sum_us'] = dict(attn_profile=sum(r['attn_profile_us'] for r in table), attn=sum(r['attn_us'] for r in table))
    assert SHARE_ONE == 2 ** 21
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(json.dumps(res, indent=1) + '\n')


if __name__ == '__main__':
    main()
