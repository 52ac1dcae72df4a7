"""VAR.class_information without a GPU: varhip_class_mix_host_f32 / varhip_class_mix_finish_host_f32, the host twins of the class-mixture
reduction (include/var_hip.h), against the numpy float64 evaluation of their definitions in tests/classinforef.py; the closed forms; the exact
invariances of the integer sums; NaN rows, out-of-range tokens, EINVAL and the ABI; class_information_torch and the public call's argument
checks on the d2 fixture model.

Bounds: derived in the docstring of tests/classinforef.py (and, for the entropy, of tests/samplestatsref.py) from the unit roundoff of fp32, the
documented accuracy of vm_exp / vm_log, one fp32 division and one rint per class."""
import math

import numpy as np
import pytest
import torch

from tests import classinforef as R
from tests import util
from tests.samplestatsref import U

OUT = ('h_mix', 'h_cond', 'mi', 'logp_mix')


def host_mix(logits, gt, images, classes, l, V, u, prior, ca=1.0, cb=0.0, acc=None, expect=0, ld_prior=None):
    """one guarded call of the twin.  acc None: the on-chip route -> dict(entropy, h_mix, h_cond, mi, logp_mix), the outputs prefilled with a
    sentinel; acc = (mix_q (images, l, V) int64, hcond_q (images, l) int64, nanflag (images, l) int32): a chunk that adds into them -> dict(entropy)"""
    from var_amd import hip
    fn = hip.lib().host['class_mix_host_f32']
    out = dict(entropy=np.full((images, classes, l), -77, np.float32))
    for k in OUT:
        out[k] = np.full((images, l), -77, np.float32)
    a = [None, None, None, 0] if acc is None else [acc[0], acc[1], acc[2], l]
    o = [out[k] for k in OUT] + [l] if acc is None else [None, None, None, None, 0]
    rc = util.guarded_invoke('varhip_class_mix_host_f32',
                             [logits, gt, l, images, classes, l, V, u, float(ca), float(cb), prior, classes if ld_prior is None else ld_prior,
                              out['entropy'], classes * l, l] + a + o, lambda *x: fn(*x))
    assert rc == expect, rc
    return out


def host_finish(acc, gt, images, l, V, expect=0):
    from var_amd import hip
    fn = hip.lib().host['class_mix_finish_host_f32']
    out = {k: np.full((images, l), -77, np.float32) for k in OUT}
    rc = util.guarded_invoke('varhip_class_mix_finish_host_f32', [acc[0], acc[1], acc[2], l, gt, l, images, l, V] + [out[k] for k in OUT] + [l],
                             lambda *x: fn(*x))
    assert rc == expect, rc
    return out


def new_acc(images, l, V):
    return np.zeros((images, l, V), np.int64), np.zeros((images, l), np.int64), np.zeros((images, l), np.int32)


def factors(u):
    t = np.float32(np.float32(1.5) * np.float32(0.5)) if u else np.float32(0)
    return np.float32(1) + t, t


def make(V, images, classes, l, u, seed, prior_seed=None):
    lg = R.synth_logits(images * (classes + u) * l, V, seed)
    gt = np.random.default_rng(seed + 1).integers(0, V, size=(images, l)).astype(np.int64)
    return lg, gt, R.make_prior(images, classes, prior_seed)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize('V', [256, 260, 4096])
@pytest.mark.parametrize('classes', [1, 2, 7])
@pytest.mark.parametrize('l,images,u,prior_seed', [(1, 1, 0, None), (5, 3, 1, 3), (5, 1, 1, None), (1, 3, 0, 4)])
def test_host_twin_against_float64(V, classes, l, images, u, prior_seed):
    lg, gt, prior = make(V, images, classes, l, u, seed=V + 10 * classes + l, prior_seed=prior_seed)
    ca, cb = factors(u)
    z = R.guided(lg, images, classes, l, V, u, ca, cb)
    ref = R.reference(z, prior, gt)
    got = host_mix(lg, gt, images, classes, l, V, u, prior, ca, cb)
    acc = new_acc(images, l, V)
    ent2 = host_mix(lg, gt, images, classes, l, V, u, prior, ca, cb, acc=acc)['entropy']
    R.check_against_reference(got, ref, f'V={V} K={classes} l={l}: ', mix_q=acc[0])
    assert np.array_equal(bits(ent2), bits(got['entropy']))
    fin = host_finish(acc, gt, images, l, V)
    for k in OUT:
        assert np.array_equal(bits(fin[k]), bits(got[k])), f'{k}: one chunk plus finish differs from the on-chip route'
    # 0 <= mi <= H(pi), up to the bound
    Hpi = -(prior.astype(np.float64) * np.log(prior.astype(np.float64))).sum(-1, keepdims=True)
    assert (got['mi'] >= -ref['mi_bound']).all() and (got['mi'] <= Hpi + ref['mi_bound']).all()
    if classes == 1:                                                        # one class with pi = 1: the mixture is the row
        assert (np.abs(got['mi']) <= ref['mi_bound']).all()


def test_one_hot_rows():
    """every class row one-hot on its own code (own logit 0, the rest -200: their exponentials are exactly 0), K = 4, uniform prior"""
    V, K, l = 256, 4, 3
    own = np.array([[5, 17, 100, 255], [0, 1, 2, 3], [9, 8, 7, 6]])          # per token the four classes' codes
    lg = np.full((K, l, V), -200, np.float32)
    for t in range(l):
        lg[np.arange(K), t, own[t]] = 0
    gt = np.array([[5, 200, 6]], np.int64)
    prior = R.make_prior(1, K)
    got = host_mix(lg.reshape(-1, V), gt, 1, K, l, V, 0, prior)
    assert (got['entropy'] == 0).all()
    acc = new_acc(1, l, V)
    host_mix(lg.reshape(-1, V), gt, 1, K, l, V, 0, prior, acc=acc)
    want = np.zeros((1, l, V), np.int64)
    for t in range(l):
        want[0, t, own[t]] = 1 << 46
    assert np.array_equal(acc[0], want) and (acc[1] == 0).all() and (acc[2] == 0).all()
    tol = 4 * U * math.log(4) + U * math.log(4)                              # one vm_log (2 ulp allowed), the final rounding
    assert (np.abs(got['mi'].astype(np.float64) - math.log(4)) <= tol).all() and (got['h_cond'] == 0).all()
    assert np.array_equal(bits(got['mi']), bits(got['h_mix']))
    assert abs(float(got['logp_mix'][0, 0]) - math.log(0.25)) <= tol and got['logp_mix'][0, 1] == -np.inf
    assert abs(float(got['logp_mix'][0, 2]) - math.log(0.25)) <= tol


def test_constant_rows():
    """constant rows at V = 256: every p_v = 2^-8 exactly, entropy = vm_log(256); the mixture of identical rows is the row: mi = 0 up to the bound"""
    V, K, l = 256, 4, 2
    lg = np.full((K * l, V), 1.25, np.float32)
    gt = np.array([[0, 255]], np.int64)
    prior = np.array([[0.5, 0.25, 0.125, 0.125]], np.float32)
    got = host_mix(lg, gt, 1, K, l, V, 0, prior)
    ref = R.reference(lg.reshape(1, K, l, V), prior, gt)
    assert (np.abs(got['entropy'].astype(np.float64) - math.log(256)) <= 5 * U * math.log(256)).all()
    assert (np.abs(got['mi']) <= ref['mi_bound']).all()
    acc = new_acc(1, l, V)
    host_mix(lg, gt, 1, K, l, V, 0, prior, acc=acc)
    assert (acc[0] == 1 << 40).all()
    R.check_against_reference(got, ref, 'constant rows: ')


def test_identical_rows():
    """all K labels' rows identical: the mixture is the row (sum pi = 1 exactly here), mi = 0 and logp_mix = the row's own log-probability"""
    V, K, l = 4096, 4, 3
    row = R.synth_logits(l, V, 7)
    lg = np.tile(row[None], (K, 1, 1)).reshape(K * l, V)
    gt = np.random.default_rng(8).integers(0, V, size=(1, l)).astype(np.int64)
    prior = np.array([[0.25, 0.5, 0.125, 0.125]], np.float32)
    got = host_mix(lg, gt, 1, K, l, V, 0, prior)
    ref = R.reference(lg.reshape(1, K, l, V), prior, gt)
    assert (np.abs(got['mi']) <= ref['mi_bound']).all()
    z64 = row.astype(np.float64)
    lp = z64 - z64.max(-1, keepdims=True)
    lp = lp - np.log(np.exp(lp).sum(-1, keepdims=True))
    own = lp[np.arange(l), gt[0]]
    assert (np.abs(got['logp_mix'][0] - own) <= ref['logp_bound'][0]).all()
    assert np.array_equal(bits(got['entropy'][0, 0]), bits(got['entropy'][0, 3]))


@pytest.mark.parametrize('V,u', [(4096, 1), (260, 0), (258, 1)])
def test_chunks_and_permutations_are_bit_equal(V, u):
    """one call over K classes == two chunked calls plus finish, bit for bit on every per-token output; a class permutation (prior permuted
    alike) leaves them bit-equal and permutes entropy"""
    images, K, l = 2, 7, 5
    lg, gt, prior = make(V, images, K, l, u, seed=21 + V, prior_seed=5)
    ca, cb = factors(u)
    cond = lg[:images * K * l].reshape(images, K, l, V)
    unc = lg[images * K * l:]
    if V <= 4096:
        whole = host_mix(lg, gt, images, K, l, V, u, prior, ca, cb)
    # chunks of 3 and 4 classes: each chunk is a pass of its own (its class rows, then the uncond rows)
    acc = new_acc(images, l, V)
    ent = []
    for k0, k1 in ((0, 3), (3, 7)):
        part = np.concatenate((np.ascontiguousarray(cond[:, k0:k1]).reshape(-1, V), unc))
        ent.append(host_mix(part, gt, images, k1 - k0, l, V, u, np.ascontiguousarray(prior[:, k0:k1]), ca, cb, acc=acc)['entropy'])
    fin = host_finish(acc, gt, images, l, V)
    if V <= 4096:
        for k in OUT:
            assert np.array_equal(bits(fin[k]), bits(whole[k])), f'{k}: chunked differs'
        assert np.array_equal(bits(np.concatenate(ent, 1)), bits(whole['entropy']))
    perm = np.array([4, 0, 6, 2, 1, 5, 3])
    lgp = np.concatenate((np.ascontiguousarray(cond[:, perm]).reshape(-1, V), unc))
    accp = new_acc(images, l, V)
    entp = host_mix(lgp, gt, images, K, l, V, u, np.ascontiguousarray(prior[:, perm]), ca, cb, acc=accp)['entropy']
    finp = host_finish(accp, gt, images, l, V)
    for k in OUT:
        assert np.array_equal(bits(finp[k]), bits(fin[k])), f'{k}: permuted classes differ'
    assert np.array_equal(accp[0], acc[0]) and np.array_equal(accp[1], acc[1])
    assert np.array_equal(bits(entp), bits(np.concatenate(ent, 1)[:, perm]))


def test_large_vocabulary_is_chunk_only():
    """V > 4096: no on-chip route (EINVAL); the chunk route and finish against float64"""
    V, images, K, l = 4100, 1, 2, 2
    lg, gt, prior = make(V, images, K, l, 0, seed=2)
    from var_amd import abi
    host_mix(lg, gt, images, K, l, V, 0, prior, expect=abi.EINVAL)
    acc = new_acc(images, l, V)
    ent = host_mix(lg, gt, images, K, l, V, 0, prior, acc=acc)['entropy']
    fin = host_finish(acc, gt, images, l, V)
    fin['entropy'] = ent
    R.check_against_reference(fin, R.reference(lg.reshape(images, K, l, V), prior, gt), 'V=4100: ', mix_q=acc[0])


@pytest.mark.parametrize('V', [256, 258])
def test_nan_row_and_out_of_range_token(V):
    images, K, l = 2, 3, 4
    lg, gt, prior = make(V, images, K, l, 0, seed=31, prior_seed=6)
    lg = lg.reshape(images, K, l, V)
    lg[0, 1, 2, 17] = np.nan                                                # image 0, class 1, token 2
    gt[1, 0], gt[1, 3], gt[0, 1] = -1, V, 1 << 40
    got = host_mix(lg.reshape(-1, V), gt, images, K, l, V, 0, prior)
    ref = R.reference(lg, prior, gt)
    assert np.isnan(got['entropy'][0, 1, 2]) and np.isnan(got['entropy']).sum() == 1
    for k in OUT:
        assert np.isnan(got[k][0, 2])
    assert np.isnan(got['logp_mix'][1, 0]) and np.isnan(got['logp_mix'][1, 3]) and np.isnan(got['logp_mix'][0, 1])
    assert np.isfinite(got['mi'][1]).all() and np.isfinite(got['h_mix'][0, 1])
    R.check_against_reference(got, ref, f'V={V}: ')
    acc = new_acc(images, l, V)
    host_mix(lg.reshape(-1, V), gt, images, K, l, V, 0, prior, acc=acc)
    assert acc[2].sum() == 1 and acc[2][0, 2] == 1
    fin = host_finish(acc, gt, images, l, V)
    for k in OUT:
        assert np.array_equal(bits(fin[k]), bits(got[k]))


def test_einval_and_abi():
    from var_amd import abi, hip
    assert 'class_mix_f32' in abi.SIGNATURES_HIP_ONLY and 'class_mix_finish_f32' in abi.SIGNATURES_HIP_ONLY
    assert abi.SIGNATURES_HOST['class_mix_host_f32'] == abi.SIGNATURES_HIP_ONLY['class_mix_f32']
    assert abi.SIGNATURES_HOST['class_mix_finish_host_f32'] == abi.SIGNATURES_HIP_ONLY['class_mix_finish_f32']
    for name in ('class_mix_f32', 'class_mix_finish_f32'):
        assert name in hip.lib().fn
    E = abi.EINVAL
    V, images, K, l = 256, 2, 2, 3
    lg, gt, prior = make(V, images, K, l, 0, seed=1)
    fn, fin = hip.lib().host['class_mix_host_f32'], hip.lib().host['class_mix_finish_host_f32']
    ent = np.zeros((images, K, l), np.float32)
    o = [np.zeros((images, l), np.float32) for _ in range(4)]
    acc = new_acc(images, l, V)
    p = lambda a: a.ctypes.data
    #       0 logits 1 gt   2 ld_gt 3 images 4 classes 5 l 6 V 7 u 8 ca 9 cb 10 prior 11 ld_prior 12 entropy 13 ld_ei 14 ld_ec
    good = [p(lg), p(gt), l, images, K, l, V, 0, 1.0, 0.0, p(prior), K, p(ent), K * l, l,
            None, None, None, 0, p(o[0]), p(o[1]), p(o[2]), p(o[3]), l]       # 15 mix_q 16 hcond_q 17 nanflag 18 ld_acc 19..22 outputs 23 ld_out
    assert fn(*good) == 0
    for pos, val in [(0, None), (1, None), (10, None), (12, None), (19, None), (20, None), (21, None), (22, None),
                     (2, l - 1), (11, K - 1), (14, l - 1), (13, K * l - 1), (23, l - 1),
                     (3, 0), (4, 0), (5, 0), (6, 0), (6, -4), (6, (1 << 24) + 1)]:
        bad = list(good); bad[pos] = val
        assert fn(*bad) == E, (pos, val)
    chunk = list(good); chunk[15:24] = [p(acc[0]), p(acc[1]), p(acc[2]), l, None, None, None, None, 0]
    assert fn(*chunk) == 0
    for pos, val in [(16, None), (17, None), (18, l - 1)]:
        bad = list(chunk); bad[pos] = val
        assert fn(*bad) == E, (pos, val)
    #        0 mix_q    1 hcond_q  2 nanflag  3 ld_acc 4 gt 5 ld_gt 6 images 7 l 8 V 9..12 outputs 13 ld_out
    goodf = [p(acc[0]), p(acc[1]), p(acc[2]), l, p(gt), l, images, l, V, p(o[0]), p(o[1]), p(o[2]), p(o[3]), l]
    assert fin(*goodf) == 0
    for pos, val in [(0, None), (1, None), (2, None), (4, None), (9, None), (10, None), (11, None), (12, None), (3, l - 1), (5, l - 1), (13, l - 1),
                     (6, 0), (7, 0), (8, 0), (8, (1 << 24) + 1)]:
        bad = list(goodf); bad[pos] = val
        assert fin(*bad) == E, (pos, val)


# ---- the PyTorch route and the public call on the d2 fixture model ------------------------------------------------------------------------
def fixture(golden_dir):
    from tests.test_token_scores_cpu import fixture_model              # (one d2 fixture model for the scoring files)
    return fixture_model(golden_dir)


@pytest.mark.parametrize('cfg', [0.0, 1.5])
def test_torch_route_against_the_restatement(golden_dir, cfg):
    """var.class_information on the d2 fixture model (CPU: class_information_torch) against the restatement of its own logits"""
    from var_amd.models.var import ClassInformation
    vae, var, meta, gt, _ = fixture(golden_dir)
    classes = [3, meta['labels'][0], 1000]
    prior = torch.tensor([0.5, 0.25, 0.25])
    r = var.class_information(gt, classes, cfg=cfg, prior=prior)
    N, K, L = 2, 3, var.L
    assert isinstance(r, ClassInformation) and r.entropy.shape == (N, K, L) and r.patch_nums == tuple(var.patch_nums)
    for k in OUT:
        assert getattr(r, k).shape == (N, L) and getattr(r, k).dtype == torch.float32
    r2 = var.class_information(gt, classes, cfg=cfg, max_rows=2, prior=prior)
    x = vae.quantize.idxBl_to_var_input([gt[:, b:e] for b, e in var.begin_ends])
    pns = meta['patch_nums']
    t = cfg * torch.tensor([si / (len(pns) - 1) for si, pn in enumerate(pns) for _ in range(pn * pn)]).view(1, -1, 1)
    for i in range(N):
        with torch.no_grad():
            z = var(torch.tensor(classes), x[i:i + 1].expand(3, -1, -1))
            if cfg > 0:
                z = (1 + t) * z - t * var(torch.tensor([var.num_classes]), x[i:i + 1])
        ref = R.reference(z.numpy()[None], r.prior[i:i + 1].numpy(), gt[i:i + 1].numpy())
        got = dict(entropy=r.entropy[i:i + 1].numpy(), **{k: getattr(r, k)[i:i + 1].numpy() for k in OUT})
        R.check_against_reference(got, ref, f'cfg {cfg} image {i}: ')
    assert r2.mi.shape == r.mi.shape and bool(torch.isfinite(r2.mi).all())     # (its rows come from other forward calls: no bitwise claim here)
    ps = r.per_scale()
    S = len(var.patch_nums)
    assert ps['mi_sum'].shape == (N, S) and ps['mi_mean'].dtype == torch.float64
    b, e = var.begin_ends[-1]
    assert torch.allclose(ps['mi_sum'][:, -1], r.mi[:, b:e].double().sum(-1)) and torch.allclose(ps['h_cond_mean'][:, 0], r.h_cond[:, 0].double())
    assert 'classes=3' in repr(r)
    m = r.mi_map(size=32)
    assert m.pred.shape == (N, 32, 32) and m.area.shape == (N, 1)


def test_torch_route_is_chunk_invariant_and_flags_nan():
    from var_amd.models.var import class_information_torch
    K, l, V = 5, 4, 64
    z = torch.from_numpy(R.synth_logits(K * l, V, 3)).view(K, l, V)
    gt = torch.tensor([0, 63, -1, 5])
    prior = torch.from_numpy(R.make_prior(1, K, 9)[0])
    a = class_information_torch(z, gt, prior)
    for mr in (1, 2, 64):
        b = class_information_torch(z, gt, prior, mr)
        assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b)), mr
    assert math.isnan(a[4][2]) and not math.isnan(a[3][2])
    ref = R.reference(z.numpy()[None], prior.numpy()[None], gt.numpy()[None])
    R.check_against_reference(dict(entropy=a[0].numpy()[None], **{k: v.numpy()[None] for k, v in zip(OUT, a[1:])}), ref, 'torch route: ')
    z[2, 1, 7] = math.nan
    c = class_information_torch(z, gt, prior, 2)
    assert math.isnan(c[0][2, 1]) and int(torch.isnan(c[0]).sum()) == 1 and all(math.isnan(v[1]) for v in c[1:]) and not math.isnan(c[3][0])


def test_prior_argument_checks(golden_dir):
    vae, var, meta, gt, _ = fixture(golden_dir)
    nan = float('nan')
    for bad in ([0.5, 0.6], [0.5, 0.4], [1.5, -0.5], [nan, 1.0], [math.inf, 0.0], [1.0], [0.2, 0.3, 0.5], [[0.5, 0.5]] * 3, [[[0.5, 0.5]]],
                [True, False], 'uniform', [0.5, 0.5 + 2e-6]):
        with pytest.raises(ValueError):
            var.class_information(gt, [1, 2], prior=bad)
    for kw in (dict(cfg=-1.0), dict(cfg=nan), dict(max_rows=0), dict(cfg=1.0, max_rows=1)):          # the token_scores checks apply
        with pytest.raises(ValueError):
            var.class_information(gt, [1, 2], **kw)
    with pytest.raises(ValueError):
        var.class_information(gt, [1, 1001])
    with pytest.raises(ValueError):
        var.class_information(gt[:1], list(range(1001)) * 17)                 # more than 16384 candidates
    # accepted: None, (K,), (N, K), a tensor, a row off 1 by less than 1e-6; used as given (rounded to fp32)
    g1 = gt[:1]
    for ok in (None, [0.25, 0.75], [[0.25, 0.75]], torch.tensor([1.0, 0.0]), np.array([0.5, 0.5 + 5e-7])):
        r = var.class_information(g1, [1, 2], prior=ok)
        assert r.prior.shape == (1, 2) and r.prior.dtype == torch.float32
    assert r.prior[0, 1].item() == float(np.float32(0.5 + 5e-7))
    one = var.class_information(g1, [1, 2], prior=[1.0, 0.0])                # all weight on one class: no information
    assert float(one.mi.abs().max()) <= 1e-5 and torch.equal(one.h_cond, one.entropy[:, 0])
