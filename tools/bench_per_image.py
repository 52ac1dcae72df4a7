#!/usr/bin/env python3
"""Timing of per-image sampling on one MI355X, random-init weights (detinit seed 0), VAR-d16 256 x 256, B = 64, cfg 1.5, top-k 900,
top-p 0.96: VAR.autoregressive_infer_cfg (the comparator, timed first) against VAR.autoregressive_infer_cfg_per_image with the same
parameters for every image, in the same process, per precision.  2 warm-up calls, --iters (>= 5) timed calls each, median, HIP events.

The fill-vs-generator line times the two noise sources alone on the largest scale's (B * 256, 4096) tensor, events around --fill-reps
back-to-back launches: varhip_exp1_philox_f32 against torch's exponential_ on the device generator, each with its write bandwidth.

    python tools/bench_per_image.py [--precisions f32,bf16] [--iters 5] [--B 64] [--out profiles/per_image_bench.json]

Prints one JSON object (and writes it to --out)."""
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

PNS = (1, 2, 3, 4, 5, 6, 8, 10, 13, 16)


def event_ms(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--precisions', default='f32,bf16')
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--B', type=int, default=64)
    ap.add_argument('--fill-reps', type=int, default=20)
    ap.add_argument('--out', default='')
    a = ap.parse_args()
    if a.iters < 5:
        ap.error('--iters must be at least 5')
    from models import build_vae_var
    B = a.B
    with contextlib.redirect_stdout(io.StringIO()):
        vae, var = build_vae_var(device='cuda', patch_nums=PNS, depth=16, ch=160)
    detinit.fill_module_device_(var, 16, 0, 'var.'); detinit.fill_module_device_(vae, 16, 0, 'vae.')
    var.eval(); vae.eval()
    labels = torch.arange(B, device='cuda') * 97 % 1000
    seeds = list(range(1000, 1000 + B))
    res = dict(config=dict(model='d16', B=B, cfg=1.5, top_k=900, top_p=0.96, warmup=2, iters=a.iters, statistic='median of HIP-event times'))
    for prec in a.precisions.split(','):
        var.set_hip_precision(prec)
        plain = event_ms(lambda: var.autoregressive_infer_cfg(B, labels, g_seed=0, cfg=1.5, top_k=900, top_p=0.96), 2, a.iters)
        per = event_ms(lambda: var.autoregressive_infer_cfg_per_image(labels, seeds, cfg=1.5, top_k=900, top_p=0.96), 2, a.iters)
        mp, mi = statistics.median(plain), statistics.median(per)
        res[prec] = dict(plain_ms=round(mp, 3), per_image_ms=round(mi, 3), per_image_over_plain=round(mi / mp, 5),
                         plain_ms_all=[round(x, 3) for x in plain], per_image_ms_all=[round(x, 3) for x in per])
        print(f'[bench_per_image] {prec}: plain {mp:.2f} ms, per-image {mi:.2f} ms ({100 * (mi / mp - 1):+.2f} %)', flush=True)
    var.set_hip_precision('f32')
    # the two noise sources alone
    rows, V, reps = B * 256, var.V, a.fill_reps
    out = torch.empty(rows, V, device='cuda')
    sd = torch.tensor(seeds, dtype=torch.int64, device='cuda')
    gen = torch.Generator(device='cuda').manual_seed(0)

    def philox():
        for _ in range(reps): hip.call('exp1_philox_f32', sd, B, 256, V, 9, 0, out)

    def torch_exp():
        for _ in range(reps): out.exponential_(1, generator=gen)
    gb = rows * V * 4 / 1e9
    fp = statistics.median(event_ms(philox, 2, a.iters)) / reps
    ft = statistics.median(event_ms(torch_exp, 2, a.iters)) / reps
    res['fill'] = dict(shape=[rows, V], philox_ms=round(fp, 4), philox_gb_s=round(gb / fp * 1e3, 1), torch_exponential_ms=round(ft, 4),
                       torch_exponential_gb_s=round(gb / ft * 1e3, 1))
    print(f'[bench_per_image] fill ({rows}, {V}): philox {fp:.4f} ms ({gb / fp * 1e3:.0f} GB/s), exponential_ {ft:.4f} ms ({gb / ft * 1e3:.0f} GB/s)', flush=True)
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
