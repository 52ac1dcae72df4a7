#!/usr/bin/env python3
"""Timing of VAR.sample_smc on one MI355X, random-init weights (detinit seed 0), VAR-d16 256 x 256, B = 8 images of n = 8 particles, cfg 1.5,
top-k 900, top-p 0.96, per precision, in one process (the protocol of tools/bench_best_of_pruned.py):
  (a) the whole call: sample_smc(resample=(4, 6), ess=None) against VAR.sample_best_of with the same arguments (equal transformer work; the SMC
      call adds two boundaries and decodes all 64 particles, so it is also timed with decode=False), the calls alternating round by round:
      2 warm-up rounds, --iters (>= 5) timed rounds, median of HIP-event times with min - max;
  (b) the boundary alone: the varhip_kv_resample launch behind scale 6 with the call's own ancestor table on the call's own caches (32 caches
      of 128 rows, 16 heads, 155 of 680 tokens), against (i) an out-of-place varhip_kv_compact of ALL rows into a second cache set and (ii) the
      torch gather (index_select on the sliced source, then a slice copy) into that second set; --reps launches between a pair of events, the
      routes alternating round by round, median per launch.  Bytes moved = rows written * heads * len * 64 * element size, read once and
      written once; the rate is given against the 6.29 TB/s a float4 copy reaches.  The memory each route needs beyond the
      call's one cache set is reported with it.

    python tools/bench_smc.py [--precisions f32,bf16] [--iters 5] [--reps 20] [--out profiles/smc_bench.json]

Prints one JSON object (and writes it to --out)."""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys

import torch

PNS = (1, 2, 3, 4, 5, 6, 8, 10, 13, 16)
KW = dict(cfg=1.5, top_k=900, top_p=0.96)
RESAMPLE = (4, 6)
HBM_COPY = 6.29e12


def rounds_ms(fns: dict, warmup: int, iters: int) -> dict:
    """every round runs each variant once, in the dict's order, each between its own pair of events -> {name: [ms per round]}"""
    out = {k: [] for k in fns}
    for r in range(warmup + iters):
        for name, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); fn(); b.record()
            torch.cuda.synchronize()
            if r >= warmup:
                out[name].append(a.elapsed_time(b))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--precisions', default='f32,bf16')
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--B', type=int, default=8)
    ap.add_argument('--n', type=int, default=8)
    ap.add_argument('--beta', type=float, default=1.0)
    ap.add_argument('--out', default='')
    a = ap.parse_args()
    if a.iters < 5:
        ap.error('--iters must be at least 5')
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from models import build_vae_var
    from var_amd import detinit, hip
    B, n = a.B, a.n
    with contextlib.redirect_stdout(io.StringIO()):
        vae, var = build_vae_var(device='cuda', patch_nums=PNS, depth=16, ch=160)
    detinit.fill_module_device_(var, 16, 0, 'var.'); detinit.fill_module_device_(vae, 16, 0, 'vae.')
    var.eval(); vae.eval()
    eng = var.engine()
    labels = torch.arange(B, device='cuda') * 97 % 1000
    seeds = [[1000 + b * n + c for c in range(n)] for b in range(B)]
    med = lambda xs: round(statistics.median(xs), 3)
    span = lambda xs: dict(median=med(xs), min=round(min(xs), 3), max=round(max(xs), 3))
    res = dict(config=dict(model='d16', B=B, n=n, resample=list(RESAMPLE), ess=None, beta=a.beta, warmup=2, iters=a.iters, reps=a.reps,
                           weights='random init (detinit seed 0)', statistic='median of HIP-event times (min - max), variants alternating per round', **KW))
    for prec in a.precisions.split(','):
        var.set_hip_precision(prec)
        smc = lambda decode: var.sample_smc(labels, seeds, resample=RESAMPLE, beta=a.beta, ess=None, max_images=B * n, decode=decode, **KW)
        ms = rounds_ms(dict(best_of=lambda: var.sample_best_of(labels, seeds, by='logp_cond', max_images=B * n, **KW),
                            smc=lambda: smc(True), smc_no_decode=lambda: smc(False)), 2, a.iters)
        r = smc(False)
        moved = [(r.ancestors[:, k] != torch.arange(n, device='cuda')).sum(1).tolist() for k in range(len(RESAMPLE))]
        out = dict(best_of_ms=span(ms['best_of']), smc_ms=span(ms['smc']), smc_no_decode_ms=span(ms['smc_no_decode']),
                   smc_over_best_of=round(med(ms['smc']) / med(ms['best_of']), 3),
                   smc_no_decode_over_best_of=round(med(ms['smc_no_decode']) / med(ms['best_of']), 3),
                   slots_overwritten_per_image=moved, ess=r.ess.tolist(), work=eng.smc_work, all={k: [round(x, 3) for x in v] for k, v in ms.items()})
        # (b) the scale-6 boundary on the caches that call just used, with its own ancestor table
        ws = next(v for k, v in eng._ws_bop.items() if k[2] == eng.precision and k[3] == 0)
        caches = ws['kc'] + ws['vc']
        R, H, L, ln = B * n, var.num_heads, var.L, var.begin_ends[RESAMPLE[1]][1]
        esz = caches[0].element_size()
        rows = (r.ancestors[:, 1] + torch.arange(B, device='cuda').view(B, 1) * n).view(-1)
        idx = torch.cat((rows, rows + R))
        idx32 = idx.to(torch.int32)
        dead = int((idx != torch.arange(2 * R, device='cuda')).sum())
        second = [torch.empty_like(t) for t in caches]                     # the second cache set the out-of-place routes need
        ptr = lambda bufs: torch.tensor([t.data_ptr() for t in bufs], dtype=torch.int64)
        cp, sp = ptr(caches), ptr(second)
        bad = torch.zeros(1, dtype=torch.int32, device='cuda')

        def resample():
            for _ in range(a.reps):
                hip.call('kv_resample', cp, len(caches), idx32, 2 * R, H, L, ln, esz, bad)

        def compact():
            for _ in range(a.reps):
                hip.call('kv_compact', cp, sp, len(caches), idx32, 2 * R, second[0].shape[0], 2 * R, H, L, ln, esz)

        def torch_gather():
            for _ in range(a.reps):
                for s, d in zip(caches, second):
                    d[:2 * R, :, :ln].copy_(s[:2 * R, :, :ln].index_select(0, idx))

        resample(); compact(); torch.cuda.synchronize()
        assert int(bad.item()) == 0
        assert all(torch.equal(s[:2 * R, :, :ln], d[:2 * R, :, :ln]) for s, d in zip(caches, second)), 'the in-place and the out-of-place result disagree'
        km = rounds_ms(dict(kv_resample=resample, kv_compact_all_rows=compact, torch_gather=torch_gather), 2, a.iters)
        us = {k: med(v) / a.reps * 1e3 for k, v in km.items()}
        row_bytes = float(H * ln * 64 * esz)
        moved_bytes = {'kv_resample': 2.0 * len(caches) * dead * row_bytes, 'kv_compact_all_rows': 2.0 * len(caches) * 2 * R * row_bytes}
        set_bytes = float(sum(t.numel() * t.element_size() for t in caches))
        rate = {k: moved_bytes[k] / (us[k] * 1e-6) for k in moved_bytes}
        out['boundary'] = dict(
            buffers=len(caches), rows=2 * R, rows_written=dead, heads=H, len=ln, Lmax=L, element_bytes=esz, cache_set_bytes=set_bytes,
            kv_resample=dict(us=round(us['kv_resample'], 2), bytes_moved=moved_bytes['kv_resample'], TBps=round(rate['kv_resample'] / 1e12, 3),
                             share_of_measured_copy_6p29TBps=round(rate['kv_resample'] / HBM_COPY, 3), extra_memory_bytes=0.0),
            kv_compact_all_rows=dict(us=round(us['kv_compact_all_rows'], 2), bytes_moved=moved_bytes['kv_compact_all_rows'],
                                     TBps=round(rate['kv_compact_all_rows'] / 1e12, 3),
                                     share_of_measured_copy_6p29TBps=round(rate['kv_compact_all_rows'] / HBM_COPY, 3), extra_memory_bytes=set_bytes),
            torch_gather=dict(us=round(us['torch_gather'], 2), bytes_moved=moved_bytes['kv_compact_all_rows'],
                              extra_memory_bytes=set_bytes + 2 * R * row_bytes, note='a second cache set plus one gathered slice at a time'),
            compact_over_resample=round(us['kv_compact_all_rows'] / us['kv_resample'], 2), torch_over_resample=round(us['torch_gather'] / us['kv_resample'], 2),
            all_ms_per_reps={k: [round(x, 3) for x in v] for k, v in km.items()})
        del second
        res[prec] = out
        print(f"[bench_smc] {prec}: best_of {med(ms['best_of']):.1f} ms, smc {med(ms['smc']):.1f} ms ({out['smc_over_best_of']:.3f}x), without decoding "
              f"{med(ms['smc_no_decode']):.1f} ms; boundary: kv_resample {us['kv_resample']:.1f} us for {dead} rows ({rate['kv_resample'] / 1e12:.2f} TB/s), "
              f"kv_compact of all rows {us['kv_compact_all_rows']:.1f} us, torch {us['torch_gather']:.1f} us", flush=True)
    var.set_hip_precision('f32')
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
