#!/usr/bin/env python3
"""Timing of the attention knockout (VAR.attention_knockout) on one MI355X, random-init weights (detinit seed 0), d16, f32, one image of 256x256
given as tokens, the default sweep (54 entries, 55 rows):

    knockout        var.attention_knockout(gt, label)                     the sweep: one pass of 55 rows, the touched (scale, block) pairs through varhip_attn_keysel_f32
    loglik          var.token_log_likelihood(gt, 55 labels)               the plain pass on as many rows (no cut anywhere, varhip_attn_cached_f32 throughout)
    torch           attention_knockout_torch on the same GPU              one batch-1 masked pass per row

alternated in one process, and the kernel alone at l = 256, curL = 680, 64 rows x 16 heads (HIP events around --reps launches, alternated --iters
times): varhip_attn_cached_f32, varhip_attn_keysel_f32 with full masks, and with one scale hidden (scale 8, 169 of the 680 keys).

    python tools/bench_attention_knockout.py [--iters 5] [--warmup 2] [--reps 20] [--out profiles/attention_knockout_bench.json]

Prints one JSON object (and writes it to --out): medians of the alternated calls with min and max."""
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
    ap.add_argument('--reps', type=int, default=20, help='launches per timing of the kernel-alone table')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    dev = torch.device('cuda', 0)
    from models import build_vae_var
    from var_amd.models import args as A
    from var_amd.models.var import attention_knockout_torch
    pns = (1, 2, 3, 4, 5, 6, 8, 10, 13, 16)
    with contextlib.redirect_stdout(io.StringIO()):
        vae, var = build_vae_var(device=dev, patch_nums=pns, depth=16, ch=160)
    detinit.fill_module_device_(var, 16, 0, 'var.'); detinit.fill_module_device_(vae, 16, 0, 'vae.')
    var.eval(); vae.eval(); var.cond_drop_rate = 0.0
    L, V, H, S = var.L, var.V, var.num_heads, len(pns)
    g = torch.Generator(device=dev).manual_seed(0)
    gt = torch.randint(0, V, (1, L), device=dev, generator=g)
    lab = torch.tensor([7], device=dev)
    edges = A.knockout_edges(None, S, tuple(range(var.depth)), tuple(range(H)), var.depth, H)
    cuts = A.knockout_masks(edges, H)
    rows = len(edges) + 1
    labs = torch.arange(rows, device=dev).unsqueeze(0)
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

    def torch_route():
        var.train()
        try:
            return attention_knockout_torch(var, gt, lab, cuts)
        finally:
            var.eval()

    def alternate(routes, reps=1):
        ms = {k: [] for k, _ in routes}
        for _ in range(a.warmup):
            for _, fn in routes:
                timed(fn, reps)
        for _ in range(a.iters):
            for k, fn in routes:
                ms[k].append(timed(fn, reps)[1])
        return {k: dict(ms_median=statistics.median(v), ms_min=min(v), ms_max=max(v)) for k, v in ms.items()}

    res = dict(images=1, entries=len(edges), rows=rows, depth=var.depth, L=L, V=V, iters=a.iters, warmup=a.warmup, reps=a.reps)
    with torch.inference_mode():
        var.set_hip_precision('f32')
        r = alternate([('knockout', lambda: var.attention_knockout(gt, lab)), ('loglik', lambda: var.token_log_likelihood(gt, labs, max_rows=64)),
                       ('torch', torch_route)])
        r['knockout']['over_loglik'] = r['knockout']['ms_median'] / r['loglik']['ms_median']
        r['torch']['over_knockout'] = r['torch']['ms_median'] / r['knockout']['ms_median']
        r['loglik']['spread'] = (r['loglik']['ms_max'] - r['loglik']['ms_min']) / r['loglik']['ms_median']
        res['call'] = r
        # the kernel alone: the last scale of the pyramid, 64 rows
        B2, l, curL = 64, pns[-1] ** 2, L
        q = torch.randn(B2 * l, H * 64, device=dev, generator=g) * 0.45
        kc, vc = torch.randn(B2, H, curL, 64, device=dev, generator=g) * 0.45, torch.randn(B2, H, curL, 64, device=dev, generator=g)
        out = torch.empty(B2 * l, H * 64, device=dev)
        ends = torch.tensor([e for _, e in var.begin_ends], dtype=torch.int32)
        full = torch.full((B2 * H,), (1 << S) - 1, dtype=torch.int32, device=dev)
        cut = torch.full((B2 * H,), ((1 << S) - 1) & ~(1 << 8), dtype=torch.int32, device=dev)
        k = alternate([('attn_cached', lambda: hip.call('attn_cached_f32', q, kc, vc, out, B2, l, H, curL, curL)),
                       ('attn_keysel_full', lambda: hip.call('attn_keysel_f32', q, kc, vc, out, B2, l, H, curL, curL, ends, S, full)),
                       ('attn_keysel_scale8_hidden', lambda: hip.call('attn_keysel_f32', q, kc, vc, out, B2, l, H, curL, curL, ends, S, cut))], a.reps)
        base = k['attn_cached']
        base['spread'] = (base['ms_max'] - base['ms_min']) / base['ms_median']
        k['attn_keysel_full']['over_attn_cached'] = k['attn_keysel_full']['ms_median'] / base['ms_median']
        k['attn_keysel_scale8_hidden']['over_attn_cached'] = k['attn_keysel_scale8_hidden']['ms_median'] / base['ms_median']
        k['attn_keysel_scale8_hidden']['visible_keys'] = curL - pns[8] ** 2
        res['kernel'] = dict(B2=B2, l=l, curL=curL, H=H, **k)
    print(json.dumps(res))
    if a.out:
        with open(a.out, 'w') as f:
            f.write(json.dumps(res, indent=1) + '\n')


if __name__ == '__main__':
    main()
