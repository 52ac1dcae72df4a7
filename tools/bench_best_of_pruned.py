#!/usr/bin/env python3
"""Timing of VAR.sample_best_of_pruned on one MI355X, random-init weights (detinit seed 0), VAR-d16 256 x 256, B = 8 images of n = 8 candidates,
cfg 1.5, top-k 900, top-p 0.96, per precision, in one process:
  (a) the pruned call at keep = {5: 2} and at keep = {4: 4, 6: 1}, each against VAR.sample_best_of with the same arguments (the unpruned call: all 64
      candidates through all ten scales), the two alternating call by call: 2 warm-up rounds, --iters (>= 5) timed rounds, median of HIP-event
      times; the share of images whose pruned winner is the unpruned winner is reported with it (random-init weights: informational only);
  (b) the boundary itself: the varhip_kv_compact launch of the {5: 2} boundary alone (32 caches of 128 rows -> 32 rows, 16 heads, 91 of 680
      tokens) on the call's own stage workspaces, against the same gather in torch on the same buffers, per block and cache
      index_select + slice copy, in two forms (index_select on the sliced source; index_select of whole rows, then the slice); --reps launches
      between a pair of events, the forms alternating round by round, median per launch.  Bytes = rows * heads * len * 64 * element size, read
      once and written once; bytes/s is given as a share of the HBM peak (8.0 TB/s specified, 6.29 TB/s measured with a float4 copy).

    python tools/bench_best_of_pruned.py [--precisions f32,bf16] [--iters 5] [--reps 20] [--out profiles/best_of_pruned_bench.json]

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
SCHEDULES = {'keep_5_2': {5: 2}, 'keep_4_4_6_1': {4: 4, 6: 1}}
HBM_SPEC, HBM_COPY = 8.0e12, 6.29e12


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
    res = dict(config=dict(model='d16', B=B, n=n, warmup=2, iters=a.iters, reps=a.reps, weights='random init (detinit seed 0)',
                           statistic='median of HIP-event times, variants alternating per round', **KW))
    for prec in a.precisions.split(','):
        var.set_hip_precision(prec)
        best_of = lambda: var.sample_best_of(labels, seeds, by='logp_cond', max_images=B * n, **KW)
        ms = {}
        for name, keep in SCHEDULES.items():          # one comparison per schedule: a stage keeps one workspace size resident, two schedules would trade it
            r = rounds_ms(dict(best_of=best_of, pruned=lambda: var.sample_best_of_pruned(labels, seeds, keep, by='logp_cond', max_images=B * n, **KW)),
                          2, a.iters)
            ms[name], ms['best_of_beside_' + name] = r['pruned'], r['best_of']
        ms['best_of'] = [x for name in SCHEDULES for x in ms['best_of_beside_' + name]]
        base = var.sample_best_of(labels, seeds, by='logp_cond', max_images=B * n, **KW)[3]
        out = dict(best_of_ms=med(ms['best_of']), all={k: [round(x, 3) for x in v] for k, v in ms.items()})
        for name, keep in SCHEDULES.items():
            r = var.sample_best_of_pruned(labels, seeds, keep, by='logp_cond', max_images=B * n, decode=False, **KW)
            out[name] = dict(keep={str(k): v for k, v in keep.items()}, pruned_ms=med(ms[name]), best_of_ms=med(ms['best_of_beside_' + name]),
                             speedup=round(med(ms['best_of_beside_' + name]) / med(ms[name]), 3),
                             same_winner_share=round(float((r.choice == base).double().mean()), 3), work=eng.best_of_work)
        # (b) the {5: 2} boundary on the stage workspaces that call just used (run it last so that they are the resident ones)
        var.sample_best_of_pruned(labels, seeds, SCHEDULES['keep_5_2'], by='logp_cond', max_images=B * n, decode=False, **KW)
        ws = {k[3]: v for k, v in eng._ws_bop.items() if k[2] == eng.precision}
        src, dst = ws[0]['kc'] + ws[0]['vc'], ws[1]['kc'] + ws[1]['vc']
        R0, R1, H, L, ln = B * n, B * 2, var.num_heads, var.L, var.begin_ends[5][1]
        esz = src[0].element_size()
        rows = torch.tensor([b * n + c for b in range(B) for c in (1, 5)], device='cuda')
        rows2 = torch.cat((rows, rows + R0))
        idx32 = rows2.to(torch.int32)
        ptr = lambda bufs: torch.tensor([t.data_ptr() for t in bufs], dtype=torch.int64)
        sp, dp = ptr(src), ptr(dst)

        def kernel():
            for _ in range(a.reps):
                hip.call('kv_compact', sp, dp, len(src), idx32, 2 * R0, dst[0].shape[0], 2 * R1, H, L, ln, esz)

        def torch_sliced():
            for _ in range(a.reps):
                for s, d in zip(src, dst):
                    d[:2 * R1, :, :ln].copy_(s[:2 * R0, :, :ln].index_select(0, rows2))

        def torch_rows():
            for _ in range(a.reps):
                for s, d in zip(src, dst):
                    d[:2 * R1, :, :ln].copy_(s[:2 * R0].index_select(0, rows2)[:, :, :ln])

        kernel(); torch.cuda.synchronize()
        want = [d[:2 * R1, :, :ln].clone() for d in dst]
        for d in dst: d[:2 * R1, :, :ln].zero_()
        torch_sliced(); torch.cuda.synchronize()
        assert all(torch.equal(d[:2 * R1, :, :ln], w) for d, w in zip(dst, want)), 'the kernel and the torch gather disagree'
        km = rounds_ms(dict(kv_compact=kernel, torch_sliced=torch_sliced, torch_rows=torch_rows), 2, a.iters)
        nbytes = 2.0 * len(src) * 2 * R1 * H * ln * 64 * esz
        us = {k: med(v) / a.reps * 1e3 for k, v in km.items()}
        rate = nbytes / (us['kv_compact'] * 1e-6)
        out['boundary'] = dict(buffers=len(src), rows_src=2 * R0, rows_out=2 * R1, heads=H, len=ln, Lmax=L, element_bytes=esz, bytes_moved=nbytes,
                               kv_compact_us=round(us['kv_compact'], 2), torch_index_select_sliced_us=round(us['torch_sliced'], 2),
                               torch_index_select_rows_us=round(us['torch_rows'], 2), kv_compact_TBps=round(rate / 1e12, 3),
                               share_of_hbm_spec_8TBps=round(rate / HBM_SPEC, 3), share_of_measured_copy_6p29TBps=round(rate / HBM_COPY, 3),
                               torch_sliced_over_kernel=round(us['torch_sliced'] / us['kv_compact'], 2),
                               torch_rows_over_kernel=round(us['torch_rows'] / us['kv_compact'], 2),
                               all_ms_per_reps={k: [round(x, 3) for x in v] for k, v in km.items()})
        res[prec] = out
        print(f"[bench_best_of_pruned] {prec}: best_of {out['best_of_ms']:.1f} ms; " +
              '; '.join(f"{k} {out[k]['pruned_ms']:.1f} ms ({out[k]['speedup']:.2f}x, same winner {out[k]['same_winner_share']:.2f})" for k in SCHEDULES) +
              f"; kv_compact {us['kv_compact']:.1f} us ({rate / 1e12:.2f} TB/s), torch {us['torch_sliced']:.1f} / {us['torch_rows']:.1f} us", flush=True)
    var.set_hip_precision('f32')
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
