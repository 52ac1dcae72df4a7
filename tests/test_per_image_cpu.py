"""Per-image sampling, the parts that need no GPU: the counter-based Exp(1) stream (Philox4x32-10 known answers, counter layout, transform,
batch independence), VAR.autoregressive_infer_cfg_per_image on the PyTorch path against the CPU oracle at B = 1, argument validation, and
two-rank sharding by seeds (gloo).  DESIGN.md §19."""
import contextlib
import io
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import util

ROOT = util.ROOT
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85


def _host(name, *args):
    from var_amd import hip
    hip.call_host(name, *args)


def philox_np(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on uint64 numpy arrays (broadcast), written from the paper's round function"""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & np.uint64(0xFFFFFFFF) for c in (c0, c1, c2, c3))
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    mask, sh = np.uint64(0xFFFFFFFF), np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2
        c0, c1, c2, c3 = (p1 >> sh) ^ c1 ^ np.uint64(k0), p1 & mask, (p0 >> sh) ^ c3 ^ np.uint64(k1), p0 & mask
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return [np.broadcast_to(c, np.broadcast(c0, c1, c2, c3).shape).astype(np.uint32) for c in (c0, c1, c2, c3)]


def host_fill(seeds, l, V, scale, draw):
    seeds = np.asarray(seeds, np.int64)
    out = np.full((len(seeds) * l, V), np.nan, np.float32)
    _host('exp1_philox_host_f32', seeds, len(seeds), l, V, scale, draw, out)
    return out


# ---- the integer stage ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('ctr, key, want', [
    ([0, 0, 0, 0], [0, 0], [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]),
    ([0xffffffff] * 4, [0xffffffff] * 2, [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]),
    ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0], [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]),
])
def test_philox4x32_10_known_answers(ctr, key, want):
    """the Random123 known-answer vectors of philox4x32_10"""
    out = np.zeros(4, np.uint32)
    _host('philox4x32_host', np.asarray(ctr, np.uint32), np.asarray(key, np.uint32), out)
    assert [hex(x) for x in out] == [hex(x) for x in want]
    assert [int(x[()]) for x in philox_np(*ctr, *key)] == want            # the numpy transcription used below agrees too


@pytest.mark.parametrize('B, l, V, scale, draw', [(1, 1, 4096, 0, 0), (3, 9, 256, 4, 1), (2, 16, 8192, 9, 0), (5, 4, 64, 2, 1)])
def test_host_fill_follows_the_documented_counter_layout(B, l, V, scale, draw):
    """key = (low, high) words of the seed, counter = (v / 4, t, scale, draw), element v = word v % 4: the fill equals, bit for bit, the
    library's transform of a numpy Philox's words at that layout; u = (2n + 1) * 2^-24 is exact (u * 2^24 is the odd integer again)"""
    seeds = [(0x0123456789abcdef * (b + 1) + b) % (1 << 63) for b in range(B)]
    got = host_fill(seeds, l, V, scale, draw).reshape(B, l, V)
    for b, sd in enumerate(seeds):
        v4, t = np.meshgrid(np.arange(V // 4), np.arange(l))
        w = np.stack(philox_np(v4, t, scale, draw, sd & 0xFFFFFFFF, sd >> 32), axis=-1).reshape(l, V)
        n = (w >> np.uint32(9)).astype(np.int64)
        u = ((2 * n + 1).astype(np.float32) * np.float32(2.0 ** -24))
        assert np.array_equal((u.astype(np.float64) * 2.0 ** 24).astype(np.int64), 2 * n + 1)              # the conversion is exact
        # the fill must be the library's transform of exactly these words (a different counter layout gives different words), ...
        e = np.empty(l * V, np.float32)
        _host('exp1_from_bits_host_f32', np.ascontiguousarray(w.reshape(-1)), l * V, e)
        assert np.array_equal(e.view(np.uint32), got[b].reshape(-1).view(np.uint32)), (b, 'fill != transform(philox words)')
        # ... and that transform is -ln u: relative error <= 2^-21 (test_transform_over_every_value_of_n) of at most 24 ln 2 < 17
        assert np.abs(got[b].astype(np.float64) + np.log(u.astype(np.float64))).max() <= 17 * 2.0 ** -21


def test_rejected_arguments():
    from var_amd import hip
    out = np.zeros(64, np.float32)
    s = np.zeros(1, np.int64)
    for B, l, V, scale, draw in [(0, 1, 4, 0, 0), (1, 0, 4, 0, 0), (1, 1, 6, 0, 0), (1, 1, 0, 0, 0), (1, 1, 4, -1, 0)]:
        with pytest.raises(hip.VarHipError, match='EINVAL'):
            _host('exp1_philox_host_f32', s, B, l, V, scale, draw, out)


# ---- the transform ----------------------------------------------------------------------------------------------------------------
# the largest relative error of e = -vm_log(u) against float64 -log(u) over all 2^23 values of n, as measured by this test
# and rounded up to the next power of two
TRANSFORM_REL_BOUND = 2.0 ** -23          # measured: 7.970527e-08 = 2^-23.58


def test_transform_over_every_value_of_n():
    n = np.arange(1 << 23, dtype=np.uint32)
    e = np.empty(n.size, np.float32)
    _host('exp1_from_bits_host_f32', n << np.uint32(9), n.size, e)
    assert np.isfinite(e).all() and (e > 0).all()
    assert (np.diff(e) <= 0).all(), 'e must be non-increasing in n'
    u = (2 * n.astype(np.float64) + 1) * 2.0 ** -24
    ref = -np.log(u)
    rel = float(np.max(np.abs(e.astype(np.float64) - ref) / ref))
    print(f'max relative error of -vm_log(u) over 2^23 values: {rel:.6e} = 2^{np.log2(rel):.3f}')
    assert rel <= 2.0 ** -21, f'vm_log is less accurate than expected on (0, 1): {rel}'
    assert rel <= TRANSFORM_REL_BOUND, rel
    # the low 9 bits of a word are not used
    e2 = np.empty(1 << 16, np.float32)
    _host('exp1_from_bits_host_f32', (n[:1 << 16] << np.uint32(9)) | np.uint32(0x1FF), 1 << 16, e2)
    assert np.array_equal(e2, e[:1 << 16])


# ---- independence -----------------------------------------------------------------------------------------------------------------
def test_an_images_rows_do_not_depend_on_the_batch():
    l, V, scale = 9, 4096, 3
    seeds = [11, 7, 1 << 40, 11 + (1 << 32), (1 << 63) - 1]
    full = host_fill(seeds, l, V, scale, 0).reshape(5, l, V)
    for b, sd in enumerate(seeds):
        alone = host_fill([sd], l, V, scale, 0).reshape(l, V)
        assert np.array_equal(alone.view(np.uint32), full[b].view(np.uint32)), b
    perm = [3, 0, 4, 2, 1]
    again = host_fill([seeds[i] for i in perm], l, V, scale, 0).reshape(5, l, V)
    for j, i in enumerate(perm):
        assert np.array_equal(again[j], full[i])
    # seed (both halves of the key), scale, row and draw all enter
    base = host_fill([11], l, V, scale, 0).reshape(l, V)
    assert not np.array_equal(base, full[1]) and not np.array_equal(base, full[3])
    assert not np.array_equal(base, host_fill([11], l, V, scale + 1, 0).reshape(l, V))
    assert not np.array_equal(base, host_fill([11], l, V, scale, 1).reshape(l, V))
    assert len({base[t].tobytes() for t in range(l)}) == l
    # a row is the same whatever l is
    assert np.array_equal(host_fill([11], 4, V, scale, 0), base[:4])


def test_mean_of_the_stream():
    N = 1 << 20
    x = host_fill([12345], N // 4096, 4096, 0, 0).astype(np.float64)
    assert x.size == N and abs(x.mean() - 1.0) <= 5 / np.sqrt(N), x.mean()
    assert abs(x.var() - 1.0) <= 0.02


# ---- the public call on the PyTorch path ------------------------------------------------------------------------------------------
PNS, DEPTH, CH = (1, 2, 3, 4), 2, 32
DECK = dict(labels=[3, 980, 22, 1000, 417], seeds=[17, 3, (1 << 62) + 5, 0, 99991], cfg=[4.0, 1.5, 0.0, 2.5, 1.5],
            top_k=[0, 900, 1, 900, 0], top_p=[0.96, 0.0, 0.0, 0.96, 0.0])


def _model():
    from models import build_vae_var
    from var_amd.detinit import fill_module_
    with contextlib.redirect_stdout(io.StringIO()):
        vae, var = build_vae_var(device='cpu', patch_nums=PNS, depth=DEPTH, ch=CH)
    fill_module_(var, DEPTH, 0, 'var.'); fill_module_(vae, DEPTH, 0, 'vae.')
    return vae, var.eval()


def _oracle():
    util.ensure_oracle_built()
    from oracle.var_oracle import OracleVAR
    meta = dict(depth=DEPTH, ch=CH, patch_nums=PNS, attn_l2_norm=True, shared_aln=False)
    var_sd, vae_sd = util.make_weights(meta)
    return OracleVAR(var_sd, vae_sd, PNS, DEPTH)


def oracle_request(orc, label, seed, cfg, top_k, top_p, more_smooth=False, V=4096):
    """the B = 1 oracle run of one request on its own host-twin noise"""
    noise = [host_fill([seed], pn * pn, V, si, 0) for si, pn in enumerate(PNS)]
    gum = [host_fill([seed], pn * pn, V, si, 1) for si, pn in enumerate(PNS)] if more_smooth else None
    return orc.run([label], noise, cfg, top_k, top_p, more_smooth=more_smooth, gumbel_noises=gum)


@pytest.mark.parametrize('more_smooth', [False, True])
def test_public_call_on_cpu_equals_the_oracle_request_by_request(more_smooth):
    vae, var = _model()
    orc = _oracle()
    d = DECK
    img, tok = var.autoregressive_infer_cfg_per_image(torch.tensor(d['labels']), d['seeds'], cfg=d['cfg'], top_k=d['top_k'], top_p=d['top_p'],
                                                      more_smooth=more_smooth, return_tokens=True)
    assert img.shape == (5, 3, 64, 64) and img.dtype == torch.float32 and tok.shape == (5, 30) and tok.dtype == torch.int64
    assert float(img.min()) >= 0.0 and float(img.max()) <= 1.0
    for b in range(5):
        ref = oracle_request(orc, d['labels'][b], d['seeds'][b], d['cfg'][b], d['top_k'][b], d['top_p'][b], more_smooth)
        assert np.array_equal(tok[b].numpy(), ref['idx'][0]), (b, tok[b].numpy(), ref['idx'][0])
        ok, msg = util.diff_report(f'image {b}', img[b].numpy(), ref['img'][0], atol=1e-3)    # (the PyTorch decoder against the oracle's: README, fp32 pixels)
        assert ok, msg


def test_scalar_and_uniform_list_parameters_agree_and_requests_are_batch_invariant():
    vae, var = _model()
    lab, seeds = [5, 6, 7], [1, 2, 3]
    a = var.autoregressive_infer_cfg_per_image(lab, seeds, cfg=2.0, top_k=900, top_p=0.96, return_tokens=True)
    b = var.autoregressive_infer_cfg_per_image(torch.tensor(lab), torch.tensor(seeds), cfg=[2.0] * 3, top_k=torch.tensor([900] * 3),
                                               top_p=np.array([0.96] * 3), return_tokens=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    alone = var.autoregressive_infer_cfg_per_image([6], [2], cfg=2.0, top_k=900, top_p=0.96, return_tokens=True)
    assert torch.equal(alone[1][0], a[1][1])
    only_img = var.autoregressive_infer_cfg_per_image(lab, seeds, cfg=2.0, top_k=900, top_p=0.96)
    assert isinstance(only_img, torch.Tensor) and torch.equal(only_img, a[0])


def test_validation():
    vae, var = _model()
    f = var.autoregressive_infer_cfg_per_image
    good = dict(label_B=[1, 2], g_seeds=[0, 1])
    f(**good, top_k=1)
    for bad in [dict(g_seeds=[0]), dict(g_seeds=[0, 1, 2]), dict(g_seeds=5), dict(cfg=[1.0]), dict(top_k=[1, 2, 3]), dict(top_p=[0.5]),
                dict(top_k=-1), dict(top_k=[0, var.V + 1]), dict(top_k=1.5), dict(top_p=-0.1), dict(top_p=[0.5, 1.01]), dict(top_p=float('nan')),
                dict(cfg=float('inf')), dict(cfg=[1.0, float('nan')]), dict(g_seeds=[0, -1]), dict(g_seeds=[0, 1 << 63]),
                dict(label_B=[1, 1001]), dict(label_B=[-1, 2]), dict(label_B=torch.tensor([0.5, 1.0])), dict(label_B=[])]:
        with pytest.raises(ValueError):
            f(**{**good, **bad})


# ---- two ranks, sharded by seeds ----------------------------------------------------------------------------------------------------
_WORKER = r'''
import contextlib, io, os, sys, torch
sys.path.insert(0, os.environ['VAR_ROOT'])
import torch.distributed as tdist
from var_amd import dist, multi
tdist.init_process_group('gloo', rank=int(os.environ['RANK']), world_size=int(os.environ['WORLD_SIZE']))
dist._state.update(rank=tdist.get_rank(), world=tdist.get_world_size(), init=True, device='cpu')
from models import build_vae_var
from var_amd.detinit import fill_module_
with contextlib.redirect_stdout(io.StringIO()):
    vae, var = build_vae_var(device='cpu', patch_nums=(1, 2, 3), depth=2, ch=32)
fill_module_(var, 2, 0, 'var.'); fill_module_(vae, 2, 0, 'vae.')
var.eval()
labels = torch.tensor([3, 980, 22, 417])
seeds, cfg, top_k, top_p = [17, 3, 5, 99991], [4.0, 1.5, 0.0, 2.5], [0, 900, 1, 900], [0.96, 0.0, 0.0, 0.96]
img, tok = multi.sample_sharded(var, 4, labels, None, cfg=cfg, top_k=top_k, top_p=top_p, g_seeds=seeds, return_tokens=True)
ref_img, ref_tok = var.autoregressive_infer_cfg_per_image(labels, seeds, cfg=cfg, top_k=top_k, top_p=top_p, return_tokens=True)
assert torch.equal(tok, ref_tok), (tok, ref_tok)
assert torch.equal(img, ref_img)
lo, hi = multi.shard_range(4, dist.get_rank(), 2)
mine = multi.sample_sharded(var, 4, labels, None, cfg=1.5, top_k=900, top_p=0.96, g_seeds=seeds, gather=False)
assert mine.shape[0] == 2 and torch.equal(mine, var.autoregressive_infer_cfg_per_image(labels[lo:hi], seeds[lo:hi], cfg=1.5, top_k=900, top_p=0.96))
try:
    multi.sample_sharded(var, 4, labels, None, cfg=cfg[:3], g_seeds=seeds)
    raise SystemExit('a parameter list of the wrong length was accepted')
except ValueError:
    pass
tdist.barrier()
print('rank', dist.get_rank(), 'ok')
'''


def test_two_rank_sharding_by_seeds_equals_the_single_process_call(tmp_path):
    script = tmp_path / 'worker.py'
    script.write_text(_WORKER)
    port = util.free_port()
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE='2', MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), VAR_ROOT=ROOT, OMP_NUM_THREADS='2')
        procs.append(subprocess.Popen([sys.executable, str(script)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = [p.communicate(timeout=300)[0] for p in procs]
    for r, (p, o) in enumerate(zip(procs, outs)):
        assert p.returncode == 0, f'rank {r} failed:\n{o}'
