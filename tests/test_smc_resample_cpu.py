"""varhip_smc_resample_host_f32 (include/var_hip.h), the host twin of the resampling decision of VAR.sample_smc, without a GPU:
bit for bit against tests/smcref.py's restatement of the contract, the invariants of systematic resampling with survivors in place, the edge
cases of the weights, unbiasedness over 4096 seeds, and every VARHIP_EINVAL.  Every array lives between guard bands (tests.util)."""
import numpy as np
import pytest

from tests import smcref as R
from tests import util

CASES = R.cases()


def twin(c, expect=0, seen=True, **over):
    """the host twin on case c (with arguments replaced by `over`) inside guard arenas -> the output arrays"""
    from var_amd import hip
    fn = hip.lib().host['smc_resample_host_f32']
    outs = ('logw', 'anc', 'did', 'ess')
    c = dict(c, **{k: v for k, v in over.items() if k not in outs})
    out = R.fresh_outputs(c, seen)
    out.update({k: v for k, v in over.items() if k in outs})
    rc = util.guarded_invoke('varhip_smc_resample_host_f32', R.call_args(c, out), lambda *a: fn(*a))
    assert rc == expect, rc
    return out


def test_philox_restatement_meets_the_published_vectors():
    from var_amd import hip
    for ctr, key, want in R.PHILOX_KAT:
        assert R.philox4x32_10(ctr, key) == want
        out = np.zeros(4, np.uint32)
        hip.call_host('philox4x32_host', np.asarray(ctr, np.uint32), np.asarray(key, np.uint32), out)
        assert out.tolist() == want


def test_vm_exp_restatement_at_known_points():
    """exp(0) = 1 exactly, 0 at and below -87, the clamp at 88, and within 2 ulp of the true value elsewhere"""
    assert R.vm_exp(0.0) == 1.0 and R.vm_exp(-87.0) == 0.0 and R.vm_exp(-1e30) == 0.0 and R.vm_exp(100.0) == R.vm_exp(88.0)
    for x in (-86.5, -20.25, -1.0, -1e-3, 0.5, 3.0):
        assert abs(float(R.vm_exp(x)) / np.exp(np.float64(np.float32(x))) - 1.0) < 2.5e-7


@pytest.mark.parametrize('c', CASES, ids=R.case_id)
def test_twin_is_the_contract_bit_for_bit(c):
    got, want = twin(c), R.ref_of(c)
    for k in R.FIELDS:
        assert R.same_bits(got[k], want[k]), (k, got[k], want[k])
    got = twin(c, seen=False)                                # logw_seen = NULL changes nothing else
    for k in ('anc', 'did', 'ess', 'logw'):
        assert R.same_bits(got[k], want[k]), k


@pytest.mark.parametrize('c', CASES, ids=R.case_id)
def test_invariants_of_every_resampled_image(c):
    got, want = twin(c), R.ref_of(c)
    n = c['n']
    anc = got['anc'].reshape(c['images'], n)
    some = False
    for i in range(c['images']):
        a = anc[i]
        assert ((0 <= a) & (a < n)).all()
        if not got['did'][i]:
            assert np.array_equal(a, np.arange(n))
            continue
        some = True
        o = np.bincount(a, minlength=n)
        w = want['w'][i]
        assert o.sum() == n and np.array_equal(o, want['offspring'][i])
        assert (np.abs(o - n * w / w.sum()) < 1).all(), (o, n * w / w.sum())          # the systematic-resampling bound
        assert np.array_equal(a[a], a)                                                # sources are fixed points
        assert all(a[k] == k for k in range(n) if o[k] >= 1)                          # survivors sit in place
        dead = [k for k in range(n) if o[k] == 0]
        assert [int(a[d]) for d in dead] == [k for k in range(n) for _ in range(o[k] - 1)]      # dead slots, ascending, take the surplus in order
        assert R.same_bits(got['logw'].reshape(-1, n)[i], np.zeros(n))                # +0.0
    if c['ess_frac'] < 0:
        assert some


def _weights_case(logw, ess_frac, images=1, seeds=None, scale=3):
    logw = np.asarray(logw, np.float64)
    n = logw.size // images
    return dict(tokens=None, ld_img=0, ld_cls=0, images=images, n=n, t0=0, t1=0, beta=1.0, logw=logw.reshape(-1),
                seeds=np.arange(images, dtype=np.int64) if seeds is None else np.asarray(seeds, np.int64), scale=scale, ess_frac=float(ess_frac))


def test_a_nan_weight_dies_whenever_the_image_resamples():
    for ess_frac in (-1.0, 1.0):
        c = _weights_case([0.5, np.nan, 0.1, -0.3, np.nan, 0.0, 0.2, -1.0], ess_frac)
        got, want = twin(c), R.ref_of(c)
        assert got['did'][0] == 1 and np.array_equal(got['anc'], want['anc'])
        assert not np.isin(got['anc'], [1, 4]).any()
        assert np.isnan(got['logw_seen'][[1, 4]]).all() and R.same_bits(got['logw'], np.zeros(8))


@pytest.mark.parametrize('logw', [[np.nan] * 4, [-np.inf] * 4, [0.0, np.inf, 1.0, np.nan], [np.inf] * 4], ids=['nan', 'minus_inf', 'one_inf', 'inf'])
def test_degenerate_images_do_not_resample(logw):
    tok = np.full(4 * 3, 0.25, np.float32)
    c = dict(_weights_case(logw, -1.0), tokens=tok, ld_img=12, ld_cls=3, t0=0, t1=3)
    got, want = twin(c), R.ref_of(c)
    assert got['did'][0] == 0 and got['ess'][0] == 0.0 and np.array_equal(got['anc'], np.arange(4))
    step1 = np.asarray(logw, np.float64) + 1.0 * 0.75
    assert R.same_bits(got['logw'], step1) and R.same_bits(got['logw_seen'], step1)
    for k in R.FIELDS:
        assert R.same_bits(got[k], want[k]), k


def test_a_degenerate_image_beside_a_healthy_one():
    c = _weights_case([np.nan, np.nan, np.nan, 0.0, 5.0, 1.0], -1.0, images=2)
    got, want = twin(c), R.ref_of(c)
    assert got['did'].tolist() == [0, 1]
    for k in R.FIELDS:
        assert R.same_bits(got[k], want[k]), k


def test_equal_weights_at_ess_frac_one_do_not_resample():
    """n = 8, w = 1: W = Q = 8, so W * W / Q == 8.0 == n exactly and 'ess < 1.0 * n' is false"""
    assert np.float64(8.0) * np.float64(8.0) / np.float64(8.0) == 8.0
    c = _weights_case([0.3] * 8, 1.0)
    got = twin(c)
    assert got['ess'][0] == 8.0 and got['did'][0] == 0 and np.array_equal(got['anc'], np.arange(8))
    assert R.same_bits(got['logw'], np.full(8, 0.3))
    assert twin(_weights_case([0.3] * 8, -1.0))['did'][0] == 1              # ... and "always" still does, to the identity
    assert np.array_equal(twin(_weights_case([0.3] * 8, -1.0))['anc'], np.arange(8))


def test_one_dominant_weight_takes_every_slot():
    for k in (0, 3, 7):
        logw = np.full(8, -2.0)
        logw[k] = 1000.0
        for ess_frac in (-1.0, 0.5):
            got = twin(_weights_case(logw, ess_frac))
            assert got['did'][0] == 1 and (got['anc'] == k).all() and got['ess'][0] == 1.0


def test_the_uniform_is_keyed_by_seed_and_scale():
    """the same weights under other seeds / scales give other tables, and the table follows from smcref's u"""
    logw = np.log(np.array([0.05, 0.3, 0.1, 0.25, 0.02, 0.08, 0.15, 0.05]))
    tabs = set()
    for seed, scale in ((1, 3), (2, 3), (1, 4), (1 << 40, 3), ((1 << 40) + 1, 3)):
        c = _weights_case(logw, -1.0, seeds=[seed], scale=scale)
        got = twin(c)
        assert np.array_equal(got['anc'], R.ref_of(c)['anc'])
        tabs.add(got['anc'].tobytes())
    assert len(tabs) > 1


def test_offspring_are_unbiased_over_4096_seeds():
    """fixed weights at n = 8, the image seeds 0 .. 4095: each o_c takes one of two adjacent integers, so its standard deviation is at most 0.5
    and the mean over 4096 independent uniforms lies within 6 * 0.5 / sqrt(4096) of n * w_c / W"""
    p = np.array([0.05, 0.3, 0.1, 0.25, 0.02, 0.08, 0.15, 0.05])
    images, n = 4096, 8
    c = _weights_case(np.tile(np.log(p), images), -1.0, images=images)
    got = twin(c)
    assert (got['did'] == 1).all()
    w = R.ref_of(_weights_case(np.log(p), -1.0))['w'][0]
    o = np.stack([np.bincount(a, minlength=n) for a in got['anc'].reshape(images, n)])
    want = n * w / w.sum()
    assert set(np.unique(o - np.floor(want)).tolist()) <= {0.0, 1.0}
    dev = np.abs(o.mean(0) - want)
    print('mean offspring', o.mean(0), 'expected', want, 'max deviation', dev.max())
    assert (dev < 6 * 0.5 / np.sqrt(4096)).all(), dev


def test_every_einval_leaves_the_outputs_alone():
    from var_amd import abi
    c = R.make_case(8, 1, -1)
    bad = [dict(n=0), dict(n=-1), dict(n=2049), dict(images=0), dict(t0=-1), dict(t1=c['t0'] - 1), dict(scale=-1), dict(ld_cls=c['t1'] - 1),
           dict(ld_img=8 * c['ld_cls'] - 1), dict(tokens=None), dict(logw=None), dict(seeds=None), dict(anc=None), dict(did=None), dict(ess=None)]
    for kw in bad:
        got = twin(c, expect=abi.EINVAL, **kw)
        fresh = R.fresh_outputs(dict(c, **{k: v for k, v in kw.items() if k not in R.FIELDS}))
        for k in R.FIELDS:
            if kw.get(k, 0) is not None:
                assert R.same_bits(got[k], fresh[k]), (kw, k)
    twin(dict(c, n=2048, images=1, t1=c['t0'], tokens=None, logw=np.zeros(2048), seeds=c['seeds'][:1]))      # the documented limit itself is accepted
