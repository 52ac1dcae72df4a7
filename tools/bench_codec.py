#!/usr/bin/env python3
"""Timing of VAR.compress / VAR.decompress on one MI355X, random-init weights (detinit seed 0), VAR-d16 256 x 256, f32, cfg 1.5, in one process:
  (a) the whole calls at B = 1, 8, 64: compress and decompress(decode=False) against the per-image sampler without its decoder
      (SamplingEngine.sample_per_image(decode=False): the same walk with the sampler as the chooser) on the same rows, the calls alternating
      round by round: 2 warm-up rounds, --iters (>= 5) timed rounds, median of HIP-event times with min - max.  compress and decompress
      include their host halves (the rANS encoder, the blob packing and parsing, the upload of the words);
  (b) the launches alone at the last scale (l = 256) on the call's own logits: varhip_code_table_f32 (pairs only, as compress calls it, and
      with cum_out, as decompress does), varhip_rans_decode_u32, and varhip_cfg_sample_rows_f32 for comparison; --reps launches between a
      pair of events, the routes alternating round by round, median per launch;
  (c) bytes per image for sampled tokens (top-k 900, top-p 0.96) and for uniform random tokens (expected near L * 12 / 8 bytes + the header).

    python tools/bench_codec.py [--iters 5] [--reps 20] [--out profiles/codec_bench.json]

Prints one JSON object (and writes it to --out)."""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys

import numpy as np
import torch

PNS = (1, 2, 3, 4, 5, 6, 8, 10, 13, 16)
CFG = 1.5


def rounds_ms(fns: dict, warmup: int, iters: int, reps: int = 1) -> dict:
    out = {k: [] for k in fns}
    for r in range(warmup + iters):
        for name, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                fn()
            b.record()
            torch.cuda.synchronize()
            if r >= warmup:
                out[name].append(a.elapsed_time(b) / reps)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--batches', default='1,8,64')
    ap.add_argument('--out', default='')
    a = ap.parse_args()
    if a.iters < 5:
        ap.error('--iters must be at least 5')
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from models import build_vae_var
    from var_amd import detinit, hip
    with contextlib.redirect_stdout(io.StringIO()):
        vae, var = build_vae_var(device='cuda', patch_nums=PNS, depth=16, ch=160)
    detinit.fill_module_device_(var, 16, 0, 'var.'); detinit.fill_module_device_(vae, 16, 0, 'vae.')
    var.eval(); vae.eval()
    eng = var.engine()
    L, V = var.L, var.V
    span = lambda xs: dict(median=round(statistics.median(xs), 3), min=round(min(xs), 3), max=round(max(xs), 3))
    res = dict(config=dict(model='d16', precision='f32', cfg=CFG, warmup=2, iters=a.iters, reps=a.reps, weights='random init (detinit seed 0)',
                           statistic='median of HIP-event times (min - max), variants alternating per round'), calls={})
    for B in [int(x) for x in a.batches.split(',')]:
        lab = torch.arange(B, device='cuda') * 97 % 1000
        seeds = [1000 + b for b in range(B)]
        tok = torch.empty(B, L, dtype=torch.int64, device='cuda')
        per = ([CFG] * B, [900] * B, [0.96] * B)
        sample = lambda: eng.sample_per_image(lab, seeds, *per, tokens_out=tok, decode=False)
        sample()
        blobs = var.compress(tok, lab, cfg=CFG).blobs
        assert torch.equal(var.decompress(blobs, decode=False).tokens, tok)
        ms = rounds_ms(dict(sample=sample, compress=lambda: var.compress(tok, lab, cfg=CFG), decompress=lambda: var.decompress(blobs, decode=False)), 2, a.iters)
        med = {k: statistics.median(v) for k, v in ms.items()}
        res['calls'][f'B={B}'] = dict(sample_no_decode_ms=span(ms['sample']), compress_ms=span(ms['compress']), decompress_no_decode_ms=span(ms['decompress']),
                                      compress_over_sample=round(med['compress'] / med['sample'], 3), decompress_over_sample=round(med['decompress'] / med['sample'], 3))
        if B == 8:
            rnd = torch.randint(0, V, (B, L), generator=torch.Generator().manual_seed(1)).cuda()
            head = 44 + 2 * len(PNS)
            res['bytes_per_image'] = dict(header=head, sampled=round(float(np.mean([len(x) for x in blobs])), 1),
                                          uniform_random=round(float(var.compress(rnd, lab, cfg=CFG).nbytes.double().mean()), 1),
                                          uniform_random_expected=round(L * 12 / 8 + head, 1), L=L)
    # (b) the launches at the last scale, on the logits the last call left (B = the last batch size)
    B = int(a.batches.split(',')[-1])
    l = PNS[-1] ** 2
    ws = eng.workspace(B)
    cum = eng._masked(ws, B, False)
    t = CFG
    gt = tok[:, L - l:].contiguous()
    pairs, flags = torch.zeros(B, l, 2, dtype=torch.int32, device='cuda'), torch.zeros(B, l, dtype=torch.int32, device='cuda')
    hip.call('code_table_f32', ws['logits'], B, l, V, t, None, gt, l, cum, pairs, flags)
    torch.cuda.synchronize()
    pr = pairs.cpu().numpy().view(np.uint32)
    streams = []
    buf, nw = np.empty(l + 2, np.uint32), np.zeros(1, np.int64)
    for b in range(B):
        hip.call_host('rans_encode_host', pr[b], l, buf, l + 2, nw)
        streams.append(buf[:int(nw[0])].copy())
    nws = np.array([len(s) for s in streams], np.int64)
    words = torch.from_numpy(np.concatenate(streams).view(np.int32)).cuda()
    off = torch.from_numpy(np.concatenate(([0], np.cumsum(nws)[:-1])).astype(np.int64)).cuda()
    nwd = torch.from_numpy(nws).cuda()
    state, err = torch.zeros(B, 4, dtype=torch.int32, device='cuda'), torch.zeros(B, dtype=torch.int32, device='cuda')
    idx = torch.empty(B * l, dtype=torch.int64, device='cuda')

    def decode():
        state.zero_(); err.zero_()
        hip.call('rans_decode_u32', cum, l, V, words, int(words.numel()), off, nwd, state, idx, err, B)
    decode()
    assert torch.equal(idx.view(B, l), gt) and not bool(err.any())
    fill = torch.empty(B * l, V, dtype=torch.float32, device='cuda').exponential_()
    masked = torch.empty(B * l, V, dtype=torch.float32, device='cuda')
    tt = torch.full((B,), t, dtype=torch.float64, device='cuda')
    tk, tp = torch.full((B,), 900, dtype=torch.int32, device='cuda'), torch.full((B,), 0.96, dtype=torch.float64, device='cuda')
    idx2 = torch.empty(B * l, dtype=torch.int64, device='cuda')
    ms = rounds_ms(dict(code_table_pairs=lambda: hip.call('code_table_f32', ws['logits'], B, l, V, t, None, gt, l, None, pairs, flags),
                        code_table_cum=lambda: hip.call('code_table_f32', ws['logits'], B, l, V, t, None, None, l, cum, None, flags),
                        rans_decode=decode,
                        cfg_sample_rows=lambda: hip.call('cfg_sample_rows_f32', ws['logits'], fill, idx2, masked, B, l, V, tt, tk, tp, 900)), 2, a.iters, a.reps)
    us = {k: round(statistics.median(v) * 1e3, 2) for k, v in ms.items()}
    hip.call('code_table_f32', ws['logits'], B, l, V, t, None, None, l, cum, None, flags)      # (the sampler's launches ran in between: leave a valid table)
    res['launches_last_scale'] = dict(B=B, l=l, V=V, us=us, span_ms={k: span(v) for k, v in ms.items()},
                                      code_table_cum_over_cfg_sample_rows=round(us['code_table_cum'] / us['cfg_sample_rows'], 3),
                                      code_table_pairs_over_cfg_sample_rows=round(us['code_table_pairs'] / us['cfg_sample_rows'], 3),
                                      rans_decode_us_per_token=round(us['rans_decode'] / l, 3),
                                      note='rans_decode includes two 1-element-per-image memsets; one wave per image, serial over the 256 tokens')
    res['unmeasured'] = ['compression ratio of a trained model (random-init weights say nothing about it)', '16-bit precisions (refused by design)',
                         'V other than 4096 and patch_nums other than the 256-pixel pyramid']
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(json.dumps(res, indent=1) + '\n')


if __name__ == '__main__':
    main()
