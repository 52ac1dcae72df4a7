#!/usr/bin/env python3
"""Timing of the per-token class information (VAR.class_information) on one MI355X, random-init weights (detinit seed 0), d16, N images of
256x256 given as tokens, K candidate classes, uniform prior, in f32 with cfg 0 and in bf16 with cfg 1.5:

    class_information  var.class_information(gt, classes, cfg=cfg)                 (every class in one pass: the mixture stays on the chip)
    chunked            var.class_information(gt, classes, cfg=cfg, max_rows=(K + 1) // 2 + u)   (two chunks per image, the global accumulator + finish)
    log_likelihood     var.token_log_likelihood(gt, classes, cfg=cfg)              (the yardstick: the same passes, one value per row)
    old                the (K, L, V) softmax route per image in torch: logits = var(label, x) (+ the unconditional forward and the guided
                       combine), softmax, the class entropies, the mixture and its entropy

all in one process; the packed routes (with the old one, on a stream of its own: it keeps its own workspace) and the two chunked routes are
alternated as two groups, because the packed and the chunked calls size the shared teacher-forced workspace differently.

    python tools/bench_class_information.py [--images 8] [--classes 10] [--iters 5] [--warmup 2] [--out profiles/class_information_bench.json]

Prints one JSON object (and writes it to --out): per configuration the median, min and max ms per call of every route (HIP events), the rise of
torch.cuda.max_memory_allocated over a call, the ratio to log_likelihood, the largest |mi| difference between the new and the old route, and
the scoring kernels' own time per call from the library's timing table (family 'sampler') for class_information, chunked and log_likelihood
with their bytes/s against the 8 TB/s HBM peak."""
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

HBM_PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=8)
    ap.add_argument('--classes', type=int, default=10)
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    dev = torch.device('cuda', 0)
    from models import build_vae_var
    pns = (1, 2, 3, 4, 5, 6, 8, 10, 13, 16)
    with contextlib.redirect_stdout(io.StringIO()):
        vae, var = build_vae_var(device=dev, patch_nums=pns, depth=16, ch=160)
    detinit.fill_module_device_(var, 16, 0, 'var.'); detinit.fill_module_device_(vae, 16, 0, 'vae.')
    var.eval(); vae.eval(); var.cond_drop_rate = 0.0
    N, K, V, L, S = a.images, a.classes, var.V, var.L, len(pns)
    g = torch.Generator(device=dev).manual_seed(0)
    gt = torch.randint(0, V, (N, L), device=dev, generator=g)
    classes = torch.randperm(1000, device=dev, generator=g)[:K]
    ratio = torch.tensor([si / (S - 1) for si, pn in enumerate(pns) for _ in range(pn * pn)], device=dev)
    ev = lambda: torch.cuda.Event(enable_timing=True)
    side = torch.cuda.Stream()

    def old_route(cfg):
        x = vae.quantize.idxBl_to_var_input([gt[:, b:e] for b, e in var.begin_ends])
        t = cfg * ratio.view(1, -1, 1)
        mi = torch.empty(N, L, device=dev)
        for i in range(N):
            z = var(classes, x[i:i + 1].expand(K, -1, -1).contiguous())
            if cfg > 0:
                z = (1 + t) * z - t * var(torch.tensor([var.num_classes], device=dev), x[i:i + 1].contiguous())
            lp = torch.log_softmax(z, dim=-1)                             # (K, L, V)
            p = lp.exp()
            h = -(p * lp).sum(-1)                                         # (K, L)
            mix = p.mean(0)                                               # (L, V)
            mi[i] = -(mix * torch.log(mix.clamp_min(1e-45))).sum(-1) - h.mean(0)
        return mi

    def timed(fn, stream):
        with torch.cuda.stream(stream):
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            e0, e1 = ev(), ev()
            e0.record()
            r = fn()
            e1.record()
            torch.cuda.synchronize()
            return r, e0.elapsed_time(e1), torch.cuda.max_memory_allocated() - base

    def kernel_time(fn):
        hip.timing_reset(); hip.timing_enable(True, ['sampler'])
        fn()
        torch.cuda.synchronize()
        tt = hip.timing_read()['sampler']
        hip.timing_enable(False)
        rate = tt['bytes'] / (tt['ms'] * 1e-3) if tt['ms'] > 0 else None
        return dict(ms_per_call=tt['ms'], launches=tt['launches'], bytes=tt['bytes'], TBps=rate / 1e12 if rate else None,
                    frac_of_hbm_peak=rate / HBM_PEAK if rate else None)

    res = dict(images=N, classes=K, depth=16, L=L, V=V, iters=a.iters, warmup=a.warmup, full_softmax_mb_per_image=K * L * V * 4 / 1e6)
    with torch.inference_mode():
        for dtype, cfg in (('f32', 0.0), ('bf16', 1.5)):
            var.set_hip_precision(dtype)
            u = int(cfg > 0)
            main_s = torch.cuda.current_stream()
            routes = [('class_information', lambda: var.class_information(gt, classes, cfg=cfg), main_s),
                      ('log_likelihood', lambda: var.token_log_likelihood(gt, classes, cfg=cfg), main_s),
                      ('chunked', lambda: var.class_information(gt, classes, cfg=cfg, max_rows=(K + 1) // 2 + u), main_s),
                      ('log_likelihood_chunked', lambda: var.token_log_likelihood(gt, classes, cfg=cfg, max_rows=(K + 1) // 2 + u), main_s),
                      ('old', lambda: old_route(cfg), side)]
            # two groups, each warmed up and alternated on its own: the packed and the chunked calls size the teacher-forced workspace
            # differently, and alternating across the groups would put its re-allocation into every timed call
            ms, peak, last = {k: [] for k, _, _ in routes}, {k: 0 for k, _, _ in routes}, {}
            for group in ((routes[0], routes[1], routes[4]), (routes[2], routes[3])):
                for _ in range(a.warmup):
                    for _, fn, st in group:
                        timed(fn, st)
                for _ in range(a.iters):                                                                     # alternated
                    for k, fn, st in group:
                        last[k], t_ms, pk = timed(fn, st)
                        ms[k].append(t_ms); peak[k] = max(peak[k], pk)
            d = {}
            for k, _, _ in routes:
                d[k] = dict(ms_median=statistics.median(ms[k]), ms_min=min(ms[k]), ms_max=max(ms[k]), peak_alloc_mb=peak[k] / 1e6)
            for k in ('class_information', 'old'):
                d[k]['over_log_likelihood'] = d[k]['ms_median'] / d['log_likelihood']['ms_median']
            d['chunked']['over_log_likelihood_chunked'] = d['chunked']['ms_median'] / d['log_likelihood_chunked']['ms_median']
            new, chk, old = last['class_information'], last['chunked'], last['old']
            d['old_vs_new'] = dict(speedup_at_median=d['old']['ms_median'] / d['class_information']['ms_median'],
                                   max_abs_mi_delta=float((new.mi - old).abs().max()), mean_mi=float(new.mi.double().mean()),
                                   chunked_bit_equal=bool(torch.equal(new.mi.view(torch.int32), chk.mi.view(torch.int32))))
            d['kernel'] = dict(class_information=kernel_time(routes[0][1]), log_likelihood=kernel_time(routes[1][1]), chunked=kernel_time(routes[2][1]),
                               log_likelihood_chunked=kernel_time(routes[3][1]))
            res[f'{dtype}_cfg{cfg:g}'] = d
        var.set_hip_precision('f32')
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(json.dumps(res, indent=1) + '\n')


if __name__ == '__main__':
    main()
