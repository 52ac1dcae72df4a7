#!/usr/bin/env python3
"""Timing of VAR.evidence_maps on one MI355X against the fork's create_heatmaps_for_classes restated in torch on the same GPU, on seeded
scores shaped like log-probabilities, patch_nums (1,2,3,4,5,6,8,10,13,16), the default scales (the first five):

    overlays   N = 8, K = 10, size = 256, an image per call: lo / hi, pred, margin, area and the (N, K, 256, 256, 3) uint8 overlays
    reduce     N = 1, K = 1000, size = 256, no maps, no overlays: lo / hi, pred, margin, area

    new        evidence_maps(...) : varhip_evidence_reduce_f32 (+ varhip_evidence_overlay_u8)
    old        the fork's procedure: per class and scale one F.interpolate(bilinear), times its weight, stack and sum over the scales; the
               global min / max; at `overlays` the normalisation, the jet colour by table lookup and the float64 blend; at `reduce` the
               arg-max, top-2 margin and bincount from the maps it has to build (K full-size maps)

both in one process, alternated, timed with device events over --iters calls after --warmup calls; the library's timing table gives the two
entry points' own time (family 'other', nothing else of it runs here), from which the overlay store's share of the HBM peak follows:
3 bytes per pixel and class written, over the overlay entry point's time.

    python tools/bench_evidence.py [--iters 20] [--warmup 3] [--out profiles/evidence_bench.json]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from var_amd import hip                                   # noqa: E402
from var_amd.models.var import evidence_maps, jet_table   # noqa: E402

HBM_PEAK = 8.0e12
PNS = (1, 2, 3, 4, 5, 6, 8, 10, 13, 16)


def old_maps(scores, size):
    """the fork's maps: a host loop over classes and scales -> (N, K, size, size)"""
    N, K, _ = scores.shape
    sel = PNS[:len(PNS) // 2]
    total = sum(p * p for p in sel)
    out = []
    for n in range(N):
        per_class = []
        for k in range(K):
            start, layers = 0, []
            for p in sel:
                up = torch.nn.functional.interpolate(scores[n, k, start:start + p * p].view(1, 1, p, p), size=(size, size), mode='bilinear',
                                                     align_corners=False).squeeze()
                layers.append(up * (p * p / total))
                start += p * p
            per_class.append(torch.stack(layers, 0).sum(0))
        out.append(torch.stack(per_class, 0))
    return torch.stack(out, 0)


def old_overlays(scores, size, image, alpha, jet):
    m = old_maps(scores, size)
    lo, hi = m.amin((1, 2, 3), keepdim=True), m.amax((1, 2, 3), keepdim=True)
    v = (m - lo) / (hi - lo)
    col = jet[(v * 256).clamp(0, 255).long()].double()
    img8 = (((image + 1) / 2) * 255).clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).unsqueeze(1).double()
    return (img8 * (1 - alpha) + col * alpha).clamp(0, 255).to(torch.uint8)


def old_reduce(scores, size):
    m = old_maps(scores, size)
    top = torch.topk(m, 2, dim=1)
    pred = top.indices[:, 0]
    return m.amin((1, 2, 3)), m.amax((1, 2, 3)), pred, top.values[:, 0] - top.values[:, 1], torch.bincount(pred.reshape(-1), minlength=m.shape[1])


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); b.synchronize()
        ms.append(a.elapsed_time(b))
    return dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms))


def kernel_ms(fn, iters):
    """the entry points' own time per call from the library's timing table"""
    hip.timing_enable(True, ['other']); hip.timing_reset()
    for _ in range(iters):
        fn()
    t = hip.timing_read()['other']
    hip.timing_enable(False)
    return t['ms'] / iters, t['launches'] // iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--old-iters', type=int, default=3)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    dev = torch.device('cuda', 0)
    L = sum(p * p for p in PNS)
    rng = np.random.default_rng(0)
    jet = jet_table().to(dev)
    res = dict(device=torch.cuda.get_device_name(0), patch_nums=list(PNS), scales=list(range(len(PNS) // 2)), iters=a.iters, old_iters=a.old_iters)

    # ---- overlays: N = 8, K = 10 ----
    N, K, size = 8, 10, 256
    scores = torch.from_numpy((-12.0 * rng.random((N, K, L))).astype(np.float32)).to(dev)
    image = torch.from_numpy((rng.random((N, 3, size, size)) * 2 - 1).astype(np.float32)).to(dev)
    new = lambda: evidence_maps(scores, PNS, size=size, image=image)                             # noqa: E731
    new_nocheck = lambda: evidence_maps(scores, PNS, size=size, image=image, check=False)        # noqa: E731
    reduce_only = lambda: evidence_maps(scores, PNS, size=size, check=False)                     # noqa: E731
    old = lambda: old_overlays(scores, size, image, 0.5, jet)                                    # noqa: E731
    got, want = new().overlays, old()
    differ = float((got != want).any(-1).float().mean())
    p = dict(N=N, K=K, size=size, new=timed(new, a.iters, a.warmup), new_check_false=timed(new_nocheck, a.iters, a.warmup),
             old=timed(old, a.old_iters, 1), pixels_differing_from_old=differ)
    both_ms, both_launches = kernel_ms(new_nocheck, a.iters)
    red_ms, red_launches = kernel_ms(reduce_only, a.iters)
    store_bytes = 3.0 * N * K * size * size
    p.update(entry_points_ms=both_ms, reduce_entry_ms=red_ms, overlay_entry_ms=both_ms - red_ms, launches_per_call=both_launches,
             overlay_store_bytes=store_bytes, overlay_store_bytes_per_s=store_bytes / ((both_ms - red_ms) * 1e-3),
             overlay_store_share_of_hbm_peak=store_bytes / ((both_ms - red_ms) * 1e-3) / HBM_PEAK,
             speedup=p['old']['median_ms'] / p['new']['median_ms'])
    res['overlays'] = p

    # ---- reduce: N = 1, K = 1000 ----
    N, K = 1, 1000
    scores = torch.from_numpy((-12.0 * rng.random((N, K, L))).astype(np.float32)).to(dev)
    new = lambda: evidence_maps(scores, PNS, size=size)                                          # noqa: E731
    new_nocheck = lambda: evidence_maps(scores, PNS, size=size, check=False)                     # noqa: E731
    old = lambda: old_reduce(scores, size)                                                       # noqa: E731
    r, o = new(), old()
    torch.cuda.reset_peak_memory_stats(); base = torch.cuda.memory_allocated(); new(); new_mem = torch.cuda.max_memory_allocated() - base
    torch.cuda.reset_peak_memory_stats(); base = torch.cuda.memory_allocated(); old(); old_mem = torch.cuda.max_memory_allocated() - base
    p = dict(N=N, K=K, size=size, new=timed(new, a.iters, a.warmup), new_check_false=timed(new_nocheck, a.iters, a.warmup),
             old=timed(old, a.old_iters, 1), pred_differing_from_old=float((r.pred[0].long() != o[2][0]).float().mean()),
             new_peak_bytes=new_mem, old_peak_bytes=old_mem)
    red_ms, red_launches = kernel_ms(new_nocheck, a.iters)
    p.update(reduce_entry_ms=red_ms, launches_per_call=red_launches, speedup=p['old']['median_ms'] / p['new']['median_ms'])
    res['reduce'] = p

    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(txt + '\n')


if __name__ == '__main__':
    main()
