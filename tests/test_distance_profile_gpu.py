"""VAR.distance_profile on the MI355X: varhip_dist_profile_f32 against the float64 restatement of tests/distprofref.py on every path (the NV 16 /
NV 4 register rows, the scalar path, partly empty workgroups, chunks, uncond rows, padded leading dimensions), its exact cases, min_prob,
accumulation and argument checks; the end-to-end call against distance_profile_torch on the engine's own d16 logits, its bitwise invariances
and the shared workspace.

Bars (tests/distprofref.py): count equal; |mass - ref| <= 1e-5 ref + count 2^-48 per cell.  Synthetic logits are generated on the CPU from
fixed seeds (the same inputs on every machine), NaN-free with |z| <= 14 after the guided combine."""
import contextlib
import math

import numpy as np
import pytest
import torch

from tests import distprofref as ref
from tests import util
from tests.test_likelihood_gpu import d16, ref_rows, tokens          # (one d16 model for the scoring files)
from var_amd import abi, hip
from var_amd.models.var import distance_profile_torch

pytestmark = pytest.mark.gpu

SENT = 1000003               # prefill of the output arrays: the kernel adds, whatever is there stays
_D = {}


def synth_dist(V, ld, seed=5):
    """a synthetic distance table [V][ld] on a grid of 1/8 in [0, 32) with a zero diagonal (values on edges happen), host and device copies"""
    if (V, ld) not in _D:
        rng = np.random.default_rng(seed)
        d = (rng.integers(0, 256, size=(V, ld)) / 8).astype(np.float32)
        d[np.arange(V), np.arange(V)] = 0
        _D[(V, ld)] = (d, torch.from_numpy(d).cuda())
    return _D[(V, ld)]


def synth_logits(rows, V, seed, scale=3.0):
    """NaN-free rows with |z| <= 5.6, so that the guided 1.75 z_c - 0.75 z_u stays within 14"""
    rng = np.random.default_rng(seed)
    return np.clip(rng.standard_normal((rows, V)) * scale, -5.6, 5.6).astype(np.float32)


def guided(lg, images, classes, l, V, u, ca, cb):
    """the fp32 z of the pass layout: a = ca * cond; b = cb * uncond; a - b (each rounded), on the device -> (images, classes, l, V) numpy"""
    cond = lg[:images * classes * l].view(images, classes, l, V)
    if not u:
        return cond.cpu().numpy()
    unc = lg[images * classes * l:].view(images, 1, l, V)
    a = torch.tensor(ca, device='cuda') * cond
    b = torch.tensor(cb, device='cuda') * unc
    return (a - b).cpu().numpy()


def off_by_4_bytes(x):
    """a copy of x that starts 4 bytes behind a 16-byte boundary"""
    buf = torch.empty(x.numel() + 1, dtype=x.dtype, device='cuda')
    v = buf[1:].view(x.shape)
    v.copy_(x)
    return v


def run(V, images, classes, l, u, edges, min_prob=0.0, pad=False, misalign=False, seed=0, gt=None, logits=None, dist=None, calls=1):
    """one guarded call (or `calls` of them into the same arrays) -> (count, mass_q as numpy (images, classes, B), z numpy, gt numpy (images, l), dist numpy)"""
    B = len(edges) - 1
    ld_dist = V + (4 if pad else 0)
    dist_h, dist_d = synth_dist(V, ld_dist) if dist is None else (dist, torch.from_numpy(dist).cuda())
    lg_h = synth_logits(images * (classes + u) * l, V, seed) if logits is None else logits
    lg = torch.from_numpy(lg_h).cuda()
    if misalign:
        lg, dist_d = off_by_4_bytes(lg), off_by_4_bytes(dist_d)
    ld_gt, tok0 = (l + 5, 3) if pad else (l, 0)
    rng = np.random.default_rng(seed + 1)
    gt_h = rng.integers(0, V, size=(images + int(pad), ld_gt)).astype(np.int64)
    if gt is not None:
        gt_h[:images, tok0:tok0 + l] = gt
    gt_d = torch.from_numpy(gt_h).cuda()
    t = np.float32(np.float32(1.5) * np.float32(0.5)) if u else np.float32(0)
    ca, cb = np.float32(1) + t, t
    # outputs: scale 1 of (images + 1, classes + 1, 2, B + 3) arrays when padded, every cell prefilled
    shape = (images + 1, classes + 1, 2, B + 3) if pad else (images, classes, 1, B)
    i0, k0, si = (1, 1, 1) if pad else (0, 0, 0)
    fill = SENT + torch.arange(int(np.prod(shape)), dtype=torch.int64, device='cuda').view(shape)
    mass, count = fill.clone(), (fill * 3).clone()
    for _ in range(calls):
        util.guarded_call('dist_profile_f32', lg, gt_d[:, tok0:], ld_gt, images, classes, l, V, u, float(ca), float(cb), dist_d, dist_d.shape[1],
                          torch.from_numpy(np.asarray(edges, np.float32)).cuda(), B, float(min_prob), mass[i0:, k0:, si], count[i0:, k0:, si],
                          shape[1] * shape[2] * shape[3], shape[2] * shape[3])
    torch.cuda.synchronize()
    dm, dc = mass - fill, count - fill * 3
    touched = torch.zeros(shape, dtype=torch.bool, device='cuda')
    touched[i0:i0 + images, k0:k0 + classes, si, :B] = True
    assert not bool(dm[~touched].any()) and not bool(dc[~touched].any()), 'the kernel wrote outside its (image, class, scale, bin) cells'
    z = guided(lg, images, classes, l, V, u, ca, cb)
    return (dc[i0:i0 + images, k0:k0 + classes, si, :B].cpu().numpy(), dm[i0:i0 + images, k0:k0 + classes, si, :B].cpu().numpy(), z,
            gt_h[:images, tok0:tok0 + l], dist_h)


E7 = [0.0, 0.125, 3.0, 7.5, 15.0, 15.125, 30.0, math.inf]        # uneven, edges on the table's grid, a last bin to +inf
E256 = np.linspace(0, 32, 257)                                     # every grid value is an edge
E1 = [4.0, 20.0]

CASES = [      # V, images, classes, l, uncond, edges, padded leading dimensions, misaligned
    (4096, 2, 3, 21, 1, E7, True, False),          # NV 16, three chunks (8 + 8 + 5), everything padded
    (4096, 1, 1, 1, 0, E256, False, False),        # one token: three of the four waves idle
    (4096, 1, 3, 4, 1, E1, False, False),
    (4096, 2, 1, 9, 0, E7, False, False),          # a full chunk and a chunk of one token
    (1024, 2, 3, 9, 1, E256, True, False),         # NV 4
    (64, 1, 3, 21, 0, E7, False, False),           # NV 4, one float4 per 16 lanes
    (64, 2, 1, 4, 1, E1, True, False),
    (4090, 2, 3, 4, 1, E7, True, False),           # V % 4 != 0: scalar path
    (4090, 1, 1, 9, 0, E256, False, False),
    (4096, 1, 3, 9, 1, E7, False, True),           # 4-byte-misaligned logits and dist: scalar path
    (1024, 2, 1, 1, 0, E1, False, True),
]


@pytest.mark.parametrize('V,images,classes,l,u,edges,pad,misalign', CASES)
def test_kernel_vs_float64(V, images, classes, l, u, edges, pad, misalign):
    c, m, z, gt, dist = run(V, images, classes, l, u, edges, pad=pad, misalign=misalign, seed=V + l)
    assert float(np.abs(z).max()) <= 14 and not np.isnan(z).any()
    wc, wm = ref.profile(z, gt, dist, np.asarray(edges, np.float32))
    ok, msg = ref.mass_ok(m, c, wc, wm)
    print(f'V={V} l={l}: {msg}')
    assert ok, msg
    assert int(wc.sum()) > 0


def test_equal_logits_are_exact():
    """rows of equal logits, V = 4096: every p_v = 2^-12, every q_v = 2^36; edges [0, inf] and min_prob 0 take every pair"""
    V, l = 4096, 9
    for u in (0, 1):
        lg = np.full((3 * (1 + u) * l, V), 2.5, np.float32)
        c, m, _, _, _ = run(V, 3, 1, l, u, [0.0, math.inf], logits=lg)
        assert (c == l * V).all(), 'edges [0, inf], min_prob 0: count == l * V'
        assert (m == c * (1 << 36)).all() and (m == l << 48).all()
        c, m, _, gt, dist = run(V, 3, 1, l, u, E7, logits=lg)
        assert (m == c * (1 << 36)).all() and int(c.sum()) == 3 * l * V
        e = np.asarray(E7, np.float32)
        want = np.array([sum(int(((dist[g, :V] >= e[b]) & (dist[g, :V] < e[b + 1])).sum()) for g in gt[i]) for i in range(3) for b in range(7)]).reshape(3, 1, 7)
        assert np.array_equal(c, want)


def test_edges_and_the_diagonal():
    """d = 0 (the diagonal) is in the first bin iff edges[0] == 0; a distance equal to an interior edge goes to the upper bin; distances at or
    above the last edge are dropped; counted with boolean masks on a table whose values sit on the edges"""
    V, l = 64, 9
    d = np.tile((np.arange(V) % 8).astype(np.float32), (V, 1))             # distances 0 .. 7, every one an integer
    d[np.arange(V), np.arange(V)] = 0
    gt = (np.arange(l) * 8 + 3) % V                                        # tokens whose own column is not a multiple of 8: the diagonal adds a zero
    n0 = np.array([(d[g] == 0).sum() for g in gt])
    assert (n0 == V // 8 + 1).all()
    for edges, first in (([0.0, 2.0, 4.0, 6.0], True), ([0.5, 2.0, 4.0, 6.0], False), ([2.0 ** -100, 2.0, 4.0, 6.0], False)):
        c, m, z, g, _ = run(V, 1, 1, l, 0, edges, gt=gt[None], dist=d)
        e = np.asarray(edges, np.float32)
        want = np.array([sum(((d[t] >= e[b]) & (d[t] < e[b + 1])).sum() for t in gt) for b in range(3)])
        assert np.array_equal(c[0, 0], want)
        # bin 0 holds the distance 1 (and 0 iff edges[0] == 0); bin 1 the distances 2 (its lower edge) and 3; 6 and 7 are dropped
        ones = sum((d[t] == 1).sum() for t in gt)
        assert c[0, 0, 0] == ones + (int(n0.sum()) if first else 0)
        assert c[0, 0, 1] == sum(((d[t] == 2) | (d[t] == 3)).sum() for t in gt) and c[0, 0, 2] == sum(((d[t] == 4) | (d[t] == 5)).sum() for t in gt)
        wc, wm = ref.profile(z, g, d, e)
        ok, msg = ref.mass_ok(m, c, wc, wm)
        assert ok, msg
    # a NaN distance is in no bin, an infinite one only below an infinite last edge ... which it is not below: dropped too
    d2 = d.copy(); d2[:, 5] = np.nan; d2[:, 6] = np.inf
    c, m, z, g, _ = run(V, 1, 1, l, 0, [0.0, math.inf], gt=gt[None], dist=d2)
    assert c[0, 0, 0] == l * (V - 2)


def test_out_of_range_tokens_add_nothing():
    l = 9
    for V in (1024, 4090):                                                  # register rows and the scalar path
        gt = np.random.default_rng(3).integers(0, V, size=(2, l)).astype(np.int64)
        gt[0, 2], gt[0, 8], gt[1, 0] = -1, V, 1 << 40
        c, m, z, g, dist = run(V, 2, 3, l, 1, E7, pad=True, gt=gt)             # (run() checks the sentinel-prefilled neighbour cells)
        wc, wm = ref.profile(z, g, dist, np.asarray(E7, np.float32))
        ok, msg = ref.mass_ok(m, c, wc, wm)
        assert ok, msg
        assert int(c[0].sum()) == 3 * (l - 2) * V and int(c[1].sum()) == 3 * (l - 1) * V
    # a scale whose every token is out of range leaves the arrays as they were
    c, m, _, _, _ = run(1024, 1, 1, 4, 0, E7, gt=np.full((1, 4), -5, np.int64))
    assert not c.any() and not m.any()


MINP_SEED = 2


def test_min_prob():
    """min_prob = 1e-10 on rows whose tails lie on both sides of it.  The input (fixed CPU seed) has no element within relative 1e-4 of the
    threshold in float64, so the fp32 p_v of the kernel is on the same side as the reference's everywhere and count must be equal."""
    V, images, classes, l = 4096, 1, 2, 6
    lg = np.clip(np.random.default_rng(MINP_SEED).standard_normal((images * classes * l, V)) * 4.5, -14, 14).astype(np.float32)
    gt = np.random.default_rng(MINP_SEED + 1).integers(0, V, size=(images, l)).astype(np.int64)
    assert ref.clear_of_threshold(lg, np.tile(gt.reshape(-1), classes), 1e-10), 'the input puts an element on the threshold: pick another seed'
    p = ref.row_probs(lg)
    below = int((p <= 1e-10).sum())
    assert 0.01 * p.size < below < 0.5 * p.size
    c, m, z, g, dist = run(V, images, classes, l, 0, E7, min_prob=1e-10, logits=lg, gt=gt)
    wc, wm = ref.profile(z, g, dist, np.asarray(E7, np.float32), 1e-10)
    assert np.array_equal(c, wc) and int(c.sum()) == p.size - below
    ok, msg = ref.mass_ok(m, c, wc, wm)
    assert ok, msg
    c0, _, _, _, _ = run(V, images, classes, l, 0, E7, logits=lg, gt=gt)
    assert int(c0.sum()) == p.size


def test_calls_accumulate():
    one = run(4096, 2, 3, 9, 1, E7, pad=True, seed=11)
    two = run(4096, 2, 3, 9, 1, E7, pad=True, seed=11, calls=2)
    assert np.array_equal(two[0], 2 * one[0]) and np.array_equal(two[1], 2 * one[1]) and one[0].any()
    again = run(4096, 2, 3, 9, 1, E7, pad=True, seed=11)
    assert np.array_equal(again[0], one[0]) and np.array_equal(again[1], one[1]), 'a repeated call differs'


def test_kernel_rejects_bad_arguments():
    V, l, B = 256, 4, 5
    lg = torch.zeros(2 * 2 * l, V, device='cuda'); gt = torch.zeros(2, 8, dtype=torch.int64, device='cuda')
    dist = torch.zeros(V, V, device='cuda'); edges = torch.arange(B + 1, dtype=torch.float32, device='cuda')
    mass = torch.zeros(2, 2, 8, dtype=torch.int64, device='cuda'); count = torch.zeros(2, 2, 8, dtype=torch.int64, device='cuda')
    f = hip.lib().fn['dist_profile_f32']
    st = hip.current_stream()
    #       0 logits       1 gt         2 ld_gt 3 images 4 classes 5 l 6 V 7 u 8 ca 9 cb 10 dist     11 ld_dist 12 edges     13 nbins 14 min_prob
    good = [lg.data_ptr(), gt.data_ptr(), 8, 2, 2, l, V, 0, 1.0, 0.0, dist.data_ptr(), V, edges.data_ptr(), B, 0.0,
            mass.data_ptr(), count.data_ptr(), 16, 8]                  # 15 mass_q  16 count  17 ld_img  18 ld_cls
    assert f(*good, st) == 0
    torch.cuda.synchronize()
    assert int(count.sum()) == 2 * 2 * l * V and int(count[..., B:].sum()) == 0      # (d = 0 everywhere: bin 0)
    for pos, val in [(0, None), (1, None), (10, None), (12, None), (15, None), (16, None),          # null pointers
                     (13, 0), (13, 257), (13, -1),                                                   # nbins outside [1, 256]
                     (18, B - 1),                                                                    # ld_cls < nbins
                     (17, 15),                                                                       # ld_img < classes * ld_cls
                     (2, l - 1),                                                                     # ld_gt < l
                     (11, V - 1),                                                                    # ld_dist < V
                     (6, 0), (6, -4), (6, (1 << 24) + 1),                                            # V outside (0, 2^24]
                     (14, float('nan')), (14, -1e-9), (14, 1.0), (14, 2.0), (14, float('inf')),      # min_prob NaN, negative or >= 1
                     (3, 0), (4, 0), (5, 0)]:                                                        # empty sizes
        a = list(good); a[pos] = val
        assert f(*a, st) == abi.EINVAL, (pos, val)
    torch.cuda.synchronize()


# ---- the model-level call -------------------------------------------------------------------------------------------
CLASSES = [1, 207, 999]


def d16_edges(var):
    dist = var.engine().code_distance_table()
    return torch.linspace(0, float(dist.max()), 100)


@contextlib.contextmanager
def precision(var, prec):
    var.set_hip_precision(prec)
    try:
        yield
    finally:
        var.set_hip_precision('f32')


@pytest.mark.parametrize('prec', ['f32', 'bf16'])
@pytest.mark.parametrize('cfg', [0.0, 1.5])
def test_d16_vs_torch_route_on_engine_logits(prec, cfg):
    """var.distance_profile against distance_profile_torch applied to var(label, x)'s logits of the same precision: counts equal (min_prob 0:
    the condition on the input is that no probability underflows, asserted on the logits' range), mass within the bar; and the mass of
    [0, inf] is l per scale within l (1e-5 + V 2^-48)"""
    vae, var = d16()
    gt = tokens(var, 2, 11)
    V, S = var.V, len(var.patch_nums)
    with precision(var, prec), torch.no_grad():
        edges = d16_edges(var)
        r = var.distance_profile(gt, CLASSES, edges, cfg=cfg)
        full = var.distance_profile(gt, CLASSES, [0.0, math.inf], cfg=cfg)
        z = ref_rows(var, vae, gt, CLASSES, cfg)                       # (N, K, L, V)
    assert r.count_NKSB.shape == (2, 3, S, 99) and r.count_NKSB.dtype == torch.int64 and r.mass_q_NKSB.dtype == torch.int64
    assert r.patch_nums == tuple(var.patch_nums) and r.count_NKSB.is_cuda
    assert float((z.amax(-1) - z.amin(-1)).max()) < 80, 'a probability could underflow in fp32: the counts would not be comparable'
    dist = var.engine().code_distance_table()
    for i in range(2):
        for si, (b, e) in enumerate(var.begin_ends):
            wc, wm = distance_profile_torch(z[i, :, b:e], gt[i, b:e], dist[gt[i, b:e]], edges, 0.0)
            ok, msg = ref.mass_ok(r.mass_q_NKSB[i, :, si].cpu().numpy(), r.count_NKSB[i, :, si].cpu().numpy(), wc.cpu().numpy(),
                                  wm.double().cpu().numpy() / ref.Q)
            assert ok, f'{prec} cfg={cfg} image {i} scale {si}: {msg}'
    for si, pn in enumerate(var.patch_nums):
        l = pn * pn
        assert bool((full.count_NKSB[:, :, si, 0] == l * V).all())
        err = (full.mass_NKSB[:, :, si, 0] - l).abs().max().item()
        assert err <= l * (1e-5 + V * 2.0 ** -48), f'{prec} cfg={cfg} scale {si}: the mass of [0, inf] is off l = {l} by {err:.3e}'
    mp = r.mean_prob(over_images=True)
    assert mp.shape == (3, S, 99) and bool(torch.isnan(mp).eq(r.count_NKSB.sum(0) == 0).all())


@pytest.mark.parametrize('prec', ['f32', 'bf16'])
def test_d16_bitwise_invariances_and_shared_workspace(prec):
    """integer accumulation: the same bits across max_rows, per-image versus packed calls, a permutation of the classes and a repeated call;
    token_log_likelihood and token_scores('expected_distance') around the call repeat bit for bit (one _tf_workspace for all of them)"""
    vae, var = d16()
    gt = tokens(var, 3, 13)
    classes = torch.tensor([[4, 90, 1000], [5, 6, 7], [999, 0, 4]], device='cuda')
    perm = torch.tensor([2, 0, 1], device='cuda')
    with precision(var, prec):
        edges = d16_edges(var)
        for cfg in (0.0, 1.5):
            u = int(cfg > 0)
            lp0 = var.token_log_likelihood(gt, classes, cfg=cfg)
            ed0 = var.token_scores(gt, classes, 'expected_distance', cfg=cfg)
            base = var.distance_profile(gt, classes, edges, cfg=cfg, max_rows=64, min_prob=1e-10)
            assert int(base.count_NKSB.sum()) > 0

            def same(r, want_c=base.count_NKSB, want_m=base.mass_q_NKSB):
                return torch.equal(r.count_NKSB, want_c) and torch.equal(r.mass_q_NKSB, want_m)
            for mr in (1 + u, 2 + u, 64):
                assert same(var.distance_profile(gt, classes, edges, cfg=cfg, max_rows=mr, min_prob=1e-10)), f'{prec} cfg={cfg} max_rows={mr}'
            singles = [var.distance_profile(gt[i:i + 1], classes[i:i + 1], edges, cfg=cfg, min_prob=1e-10) for i in range(3)]
            assert torch.equal(torch.cat([s.count_NKSB for s in singles]), base.count_NKSB), f'{prec} cfg={cfg}: per-image calls differ'
            assert torch.equal(torch.cat([s.mass_q_NKSB for s in singles]), base.mass_q_NKSB), f'{prec} cfg={cfg}: per-image calls differ'
            permuted = var.distance_profile(gt, classes[:, perm], edges, cfg=cfg, min_prob=1e-10)
            assert same(permuted, base.count_NKSB[:, perm], base.mass_q_NKSB[:, perm]), f'{prec} cfg={cfg}: permuted classes'
            assert torch.equal(var.token_log_likelihood(gt, classes, cfg=cfg), lp0), 'token_log_likelihood changed after distance_profile'
            assert torch.equal(var.token_scores(gt, classes, 'expected_distance', cfg=cfg), ed0), 'expected_distance changed after distance_profile'
