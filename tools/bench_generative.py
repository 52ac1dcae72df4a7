#!/usr/bin/env python3
"""Timing of VAR as a generative zero-shot classifier (fork eval_prob.py --mode gen) on one MI355X, random-init weights (detinit seed 0),
N images of 256x256, d16, K classes, --cfg, --clayer c:

    new route   VAR.classify_generative(img, classes, c, feature, cfg)     (N x K rows packed into passes of <= --max-rows rows)
    old route   per image (eval_prob.py:466-516): var.inpainting(gt.repeat(K), mask.repeat(K), cfg, top_k=1, top_p=0, label=classes)
                with gt = vae.img_to_idxBl(img), then img_to_post / img_to_fhat(...)[-1] of the input and of the K reconstructions and the
                torch L1 (vae.img_to_* are fp32 in every mode; the old route's transformer and decoder follow set_hip_precision)

per precision (f32, f16, bf16) and feature (vae_post, vae_fhat).  The new route's per-stage milliseconds come from one extra call with
engine.profile_generative set (an event pair and a sync around every stage: image side, AR loop, decode, encode, quantize, distance).

    python tools/bench_generative.py [--images 64] [--k 10] [--cfg 4] [--clayer 4] [--max-rows 64] [--iters 2] [--precisions f32,f16,bf16]

Prints one JSON object: per (precision, feature): images/s and ms per image of both routes, their ratio, the stage table, the peak
allocation of the new route and how often the two routes' pred agree."""
import argparse
import contextlib
import io
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from var_amd import detinit      # noqa: E402

PNS = (1, 2, 3, 4, 5, 6, 8, 10, 13, 16)


def old_route(var, vae, img, classes, c, feat, cfg):
    N, K = img.shape[0], classes.numel()
    keep_n = var.begin_ends[c][1]
    score = torch.empty(N, K, device='cuda')
    with torch.inference_mode():
        for n in range(N):
            x = img[n:n + 1]
            gt = torch.cat(vae.img_to_idxBl(x), 1)
            mask = torch.ones_like(gt); mask[:, keep_n:] = 0
            out = var.inpainting(gt.repeat(K, 1), mask.repeat(K, 1).bool(), cfg=cfg, top_k=1, top_p=0, label=classes)
            if feat == 'vae_fhat':
                fi, fr = vae.img_to_fhat(x)[-1], vae.img_to_fhat(out)[-1]
            else:
                fi, fr = vae.img_to_post(x), vae.img_to_post(out)
            score[n] = -torch.abs(fi.view(1, -1) - fr.view(K, -1)).mean(dim=-1)
    return score


def timed(fn, iters):
    torch.cuda.synchronize()
    best = float('inf')
    out = None
    for _ in range(iters):
        t0 = time.perf_counter(); out = fn(); torch.cuda.synchronize(); best = min(best, time.perf_counter() - t0)
    return best, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=64)
    ap.add_argument('--k', type=int, default=10)
    ap.add_argument('--cfg', type=float, default=4.0)
    ap.add_argument('--clayer', type=int, default=4)
    ap.add_argument('--max-rows', type=int, default=64)
    ap.add_argument('--iters', type=int, default=2)
    ap.add_argument('--precisions', default='f32,f16,bf16')
    ap.add_argument('--features', default='vae_post,vae_fhat')
    ap.add_argument('--no-old', action='store_true', help='time the new route only')
    a = ap.parse_args()
    from models import build_vae_var
    with contextlib.redirect_stdout(io.StringIO()):
        vae, var = build_vae_var(device='cuda', patch_nums=PNS, depth=16, ch=160)
    detinit.fill_module_device_(var, 16, 0, 'var.'); detinit.fill_module_device_(vae, 16, 0, 'vae.')
    var.eval(); vae.eval()
    g = torch.Generator(device='cuda').manual_seed(0)
    img = torch.rand(a.images, 3, 256, 256, device='cuda', generator=g) * 2 - 1
    classes = torch.arange(a.k, device='cuda') * 97 % 1000
    eng = var.engine()
    res = dict(tool='bench_generative', model='d16', images=a.images, k=a.k, cfg=a.cfg, clayer=a.clayer, max_rows=a.max_rows, runs={})
    for prec in a.precisions.split(','):
        var.set_hip_precision(prec)
        for feat in a.features.split(','):
            new = lambda: var.classify_generative(img, classes, a.clayer, feat, cfg=a.cfg, max_rows=a.max_rows)
            new()                                                               # warm-up (workspaces, 16-bit weight copies)
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.max_memory_allocated()
            t_new, r = timed(new, a.iters)
            peak = torch.cuda.max_memory_allocated() - base
            eng.profile_generative = True
            new()
            stages = {k: round(v / a.images, 3) for k, v in eng.generative_ms.items()}
            eng.profile_generative = False
            run = dict(new_ms_per_image=round(1e3 * t_new / a.images, 3), new_images_per_s=round(a.images / t_new, 3),
                       new_stage_ms_per_image=stages, new_peak_alloc_gb=round(peak / 1e9, 3))
            if not a.no_old:
                old = lambda: old_route(var, vae, img, classes, a.clayer, feat, a.cfg)
                old()
                t_old, s_old = timed(old, max(1, a.iters - 1))
                run.update(old_ms_per_image=round(1e3 * t_old / a.images, 3), old_images_per_s=round(a.images / t_old, 3),
                           speedup=round(t_old / t_new, 3), pred_agree=float((s_old.argmax(-1) == r.pred).float().mean()))
            res['runs'][f'{prec}/{feat}'] = run
            print(json.dumps({f'{prec}/{feat}': run}), file=sys.stderr, flush=True)
    var.set_hip_precision('f32')
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
