#!/usr/bin/env python3
"""Timing of VQVAE.forward on one MI355X, random-init weights (detinit seed 0), the d16 tokenizer (ch 160, 10 scales), B = 64, 256 x 256, fp32.
Three routes in one process, 2 warm-up calls and --iters (>= 5) timed calls each, median of HIP-event times:

  a  vae(img, ret_usages=True)                                              (the usages' .item() calls included)
  b  what a user had to hand-build before: img_to_fhat + img_to_idxBl + img_to_post (three encodes) + per-scale torch.bincount and F.mse_loss + fhat_to_img
     — API and code this feature does not touch: the comparator
  c  img_to_reconstructed_img(last_one=True): encode + quantise + decode, the floor

    python tools/bench_vae_forward.py [--iters 5] [--B 64] [--out profiles/vae_forward_bench.json]

Prints one JSON object (and writes it to --out)."""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from var_amd import detinit      # noqa: E402
from bench_per_image import event_ms      # noqa: E402

PNS = (1, 2, 3, 4, 5, 6, 8, 10, 13, 16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--B', type=int, default=64)
    ap.add_argument('--out', default='')
    a = ap.parse_args()
    if a.iters < 5:
        ap.error('--iters must be at least 5')
    from models import build_vae_var
    with contextlib.redirect_stdout(io.StringIO()):
        vae, _ = build_vae_var(device='cuda', patch_nums=PNS, depth=2, ch=160)
    detinit.fill_module_device_(vae, 16, 0, 'vae.')
    vae.eval()
    B, V = a.B, vae.vocab_size
    img = torch.rand(B, 3, 256, 256, generator=torch.Generator().manual_seed(0)).cuda() * 2 - 1

    def route_a():
        return vae(img, ret_usages=True)

    def route_b():
        fhs = vae.img_to_fhat(img)
        idx = vae.img_to_idxBl(img)
        f = vae.img_to_post(img)                                    # (f is in neither call's output: img_to_post is a third encode)
        hits = torch.stack([torch.bincount(i.reshape(-1), minlength=V) for i in idx])
        loss = 0.0
        for fh in fhs:
            m = F.mse_loss(fh, f)
            loss = loss + (m * vae.quantize.beta + m)
        loss = loss * (1. / len(fhs))
        q = vae.quantize
        margin = 1 * (f.numel() / f.shape[1]) / V * 0.08
        usages = [(q.ema_vocab_hit_SV[si] >= margin).float().mean().item() * 100 for si in range(len(PNS))]
        return vae.fhat_to_img(fhs[-1]), usages, loss, hits

    def route_c():
        return vae.img_to_reconstructed_img(img, last_one=True)

    with torch.inference_mode():
        tb = event_ms(route_b, 2, a.iters)                          # the comparator first
        ta = event_ms(route_a, 2, a.iters)
        tc = event_ms(route_c, 2, a.iters)
    ma, mb, mc = (statistics.median(t) for t in (ta, tb, tc))
    res = dict(config=dict(model='d16 tokenizer (ch 160)', B=B, image=256, precision='f32', warmup=2, iters=a.iters, statistic='median of HIP-event times'),
               forward_ms=round(ma, 3), hand_built_ms=round(mb, 3), reconstruct_ms=round(mc, 3), forward_over_hand_built=round(ma / mb, 5),
               stats_cost_ms=round(ma - mc, 3), stats_cost_share_of_reconstruct=round((ma - mc) / mc, 5),
               forward_ms_all=[round(x, 3) for x in ta], hand_built_ms_all=[round(x, 3) for x in tb], reconstruct_ms_all=[round(x, 3) for x in tc])
    print(f'[bench_vae_forward] forward {ma:.2f} ms, hand-built {mb:.2f} ms, reconstruct {mc:.2f} ms; statistics cost {ma - mc:+.3f} ms '
          f'({100 * (ma - mc) / mc:+.2f} % of reconstruct)', flush=True)
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
