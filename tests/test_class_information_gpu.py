"""VAR.class_information on the MI355X: varhip_class_mix_f32 / varhip_class_mix_finish_f32 against their host twins bit for bit on every path
(the NV 16 / NV 4 register rows with and without guidance, more classes than waves, the memory path, V > 4096, padded leading dimensions, the
on-chip route and the chunked route with finish, a NaN row, out-of-range tokens), a misaligned operand against float64, the argument checks;
the end-to-end call on the d16 model against the float64 restatement and class_information_torch on the engine's own logits, its bitwise
invariances and the shared workspace.

Bounds: tests/classinforef.py.  Synthetic logits are generated on the CPU from fixed seeds (the same inputs on every machine)."""
import numpy as np
import pytest
import torch

from tests import classinforef as R
from tests import util
from tests.test_distance_profile_gpu import off_by_4_bytes, precision
from tests.test_likelihood_gpu import d16, ref_rows, tokens          # (one d16 model for the scoring files)
from var_amd import abi, hip
from var_amd.models.var import class_information_torch

pytestmark = pytest.mark.gpu

OUT = ('h_mix', 'h_cond', 'mi', 'logp_mix')
SENT = -77.0


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def factors(u):
    t = np.float32(np.float32(1.5) * np.float32(0.5)) if u else np.float32(0)
    return float(np.float32(1) + t), float(t)


class Case:
    """the operands of one pass as numpy arrays, padded leading dimensions when pad"""
    def __init__(self, V, images, classes, l, u, prior_seed=None, pad=False, seed=0, logits=None, gt=None):
        self.V, self.images, self.classes, self.l, self.u = V, images, classes, l, u
        self.lg = R.synth_logits(images * (classes + u) * l, V, seed) if logits is None else logits
        p = 3 if pad else 0
        self.ld_gt, self.ld_prior, self.ld_ec, self.ld_out, self.ld_acc = l + p, classes + p, l + p, l + p, l + p
        self.gt = np.random.default_rng(seed + 1).integers(0, V, size=(images, self.ld_gt)).astype(np.int64)
        if gt is not None:
            self.gt[:, :l] = gt
        self.prior = np.full((images, self.ld_prior), 0.5, np.float32)
        self.prior[:, :classes] = R.make_prior(images, classes, prior_seed)
        self.ca, self.cb = factors(u)

    def z(self):
        return R.guided(self.lg, self.images, self.classes, self.l, self.V, self.u, self.ca, self.cb)

    def outputs(self, classes=None):
        k = self.classes if classes is None else classes
        return dict(entropy=np.full((self.images, k, self.ld_ec), SENT, np.float32), **{n: np.full((self.images, self.ld_out), SENT, np.float32) for n in OUT})

    def acc(self):
        return (np.zeros((self.images, self.ld_acc, self.V), np.int64), np.zeros((self.images, self.ld_acc), np.int64),
                np.zeros((self.images, self.ld_acc), np.int32))

    def rows(self, k0, k1):
        """the pass of the classes [k0, k1): their rows, then the uncond rows"""
        i, K, l, V = self.images, self.classes, self.l, self.V
        cond = self.lg[:i * K * l].reshape(i, K, l, V)[:, k0:k1]
        return np.concatenate((np.ascontiguousarray(cond).reshape(-1, V), self.lg[i * K * l:]))


def call_mix(c, host, lg, prior, nk, out, acc, misalign=False):
    """one varhip_class_mix(_host)_f32 call on numpy operands (host) or their device copies (guarded); results land in out / acc (numpy)"""
    a = [None, None, None, 0] if acc is None else [acc[0], acc[1], acc[2], c.ld_acc]
    o = [out[n] for n in OUT] + [c.ld_out] if acc is None else [None, None, None, None, 0]
    args = [lg, c.gt, c.ld_gt, c.images, nk, c.l, c.V, c.u, c.ca, c.cb, prior, c.ld_prior, out['entropy'], nk * c.ld_ec, c.ld_ec] + a + o
    if host:
        f = hip.lib().host['class_mix_host_f32']
        rc = f(*[x.ctypes.data if isinstance(x, np.ndarray) else x for x in args])
        assert rc == 0, rc
        return
    dev = [torch.from_numpy(x).cuda() if isinstance(x, np.ndarray) else x for x in args]
    if misalign:
        dev[0] = off_by_4_bytes(dev[0])
    util.guarded_call('class_mix_f32', *dev)
    torch.cuda.synchronize()
    for x, d in zip(args, dev):
        if isinstance(x, np.ndarray) and x is not lg and x is not c.gt and x is not prior:
            x[...] = d.cpu().numpy()


def call_finish(c, host, acc, out):
    args = [acc[0], acc[1], acc[2], c.ld_acc, c.gt, c.ld_gt, c.images, c.l, c.V] + [out[n] for n in OUT] + [c.ld_out]
    if host:
        rc = hip.lib().host['class_mix_finish_host_f32'](*[x.ctypes.data if isinstance(x, np.ndarray) else x for x in args])
        assert rc == 0, rc
        return
    dev = [torch.from_numpy(x).cuda() if isinstance(x, np.ndarray) else x for x in args]
    util.guarded_call('class_mix_finish_f32', *dev)
    torch.cuda.synchronize()
    for n, d in zip(OUT, dev[9:13]):
        out[n][...] = d.cpu().numpy()


def both_routes(c, host, split):
    """-> (on-chip outputs or None, chunked outputs, accumulator): the on-chip route over all classes (V <= 4096) and the chunked route over
    the classes [0, split) and [split, K) plus finish"""
    whole = None
    if c.V <= 4096:
        whole = c.outputs()
        call_mix(c, host, c.lg, c.prior, c.classes, whole, None)
    acc, ch = c.acc(), c.outputs()
    ents = []
    for k0, k1 in ((0, split), (split, c.classes)):
        if k1 > k0:
            o = c.outputs(k1 - k0)
            pr = np.full_like(c.prior, 0.5)                              # the chunk's priors first, the leading dimension kept
            pr[:, :k1 - k0] = c.prior[:, k0:k1]
            call_mix(c, host, c.rows(k0, k1), pr, k1 - k0, o, acc)
            ents.append(o['entropy'])
    ch['entropy'] = np.concatenate(ents, 1)
    call_finish(c, host, acc, ch)
    return whole, ch, acc


def same(a, b, what):
    for n in ('entropy',) + OUT:
        assert np.array_equal(bits(a[n]), bits(b[n])), f'{what}: {n} differs'


CASES = [      # V, images, classes, l, uncond, prior seed, padded leading dimensions, split
    (4096, 2, 7, 5, 1, 3, True, 3),            # NV 16 with guidance, a wave takes two rows (the prefetch), everything padded
    (4096, 1, 1, 1, 0, None, False, 1),        # one row: three of the four waves idle, the second chunk empty
    (4096, 1, 9, 3, 0, 4, False, 4),           # wave 0 takes three rows
    (1024, 2, 2, 5, 1, None, True, 1),         # NV 4
    (256, 3, 7, 5, 0, 5, False, 2),
    (260, 1, 7, 5, 1, None, True, 6),          # NV 4, the last float4 row partly filled
    (258, 2, 7, 3, 1, 6, True, 3),             # V % 4 != 0: the memory path
    (4100, 1, 2, 2, 0, None, False, 1),        # V > 4096: chunks only, global integer atomics
]


@pytest.mark.parametrize('V,images,classes,l,u,prior_seed,pad,split', CASES)
def test_kernel_equals_host_twin(V, images, classes, l, u, prior_seed, pad, split):
    c = Case(V, images, classes, l, u, prior_seed, pad, seed=V + classes)
    hw, hc, hacc = both_routes(c, True, split)
    gw, gc, gacc = both_routes(c, False, split)
    same(gc, hc, 'chunked route, kernel vs twin')
    assert np.array_equal(gacc[0], hacc[0]) and np.array_equal(gacc[1], hacc[1]) and np.array_equal(gacc[2], hacc[2])
    if hw is not None:
        same(gw, hw, 'on-chip route, kernel vs twin')
        same(gw, gc, 'on-chip vs chunked route')
    # nothing outside the (image, class, token) cells was written
    for o in (gw, gc):
        if o is not None:
            assert (o['entropy'][:, :, l:] == SENT).all() and all((o[n][:, l:] == SENT).all() for n in OUT)
    assert not gacc[0][:, l:].any() and not gacc[1][:, l:].any() and not gacc[2][:, l:].any()
    ref = R.reference(c.z(), c.prior[:, :classes], c.gt[:, :l])
    R.check_against_reference({n: v[..., :l] for n, v in gc.items()}, ref, f'V={V}: ', mix_q=gacc[0][:, :l])


@pytest.mark.parametrize('V', [4096, 1024])
def test_misaligned_logits_take_the_memory_path(V):
    """logits 4 bytes behind a 16-byte boundary: the memory path, another summation order than the twin's: held to the float64 bounds"""
    c = Case(V, 2, 5, 3, 1, 7, seed=V + 1)
    o = c.outputs()
    call_mix(c, False, c.lg, c.prior, c.classes, o, None, misalign=True)
    R.check_against_reference(o, R.reference(c.z(), c.prior, c.gt), f'misaligned V={V}: ')


@pytest.mark.parametrize('V', [4096, 258])
def test_nan_row_and_out_of_range_tokens(V):
    images, K, l = 2, 6, 4
    lg = R.synth_logits(images * K * l, V, 41).reshape(images, K, l, V)
    lg[0, 5, 2, 17] = np.nan
    gt = np.random.default_rng(42).integers(0, V, size=(images, l)).astype(np.int64)
    gt[1, 0], gt[1, 3], gt[0, 1] = -1, V, 1 << 40
    c = Case(V, images, K, l, 0, 8, logits=lg.reshape(-1, V), gt=gt)
    hw, hc, hacc = both_routes(c, True, 2)
    gw, gc, gacc = both_routes(c, False, 2)
    same(gw, hw, 'on-chip'); same(gc, hc, 'chunked'); same(gw, gc, 'routes')
    assert np.array_equal(gacc[2], hacc[2]) and gacc[2].sum() == 1 and gacc[2][0, 2] == 1
    assert np.isnan(gw['entropy'][0, 5, 2]) and np.isnan(gw['entropy']).sum() == 1
    assert all(np.isnan(gw[n][0, 2]) for n in OUT)
    assert np.isnan(gw['logp_mix'][1, 0]) and np.isnan(gw['logp_mix'][1, 3]) and np.isnan(gw['logp_mix'][0, 1])
    assert np.isfinite(gw['mi'][1]).all() and np.isfinite(gw['mi'][0, 1])
    R.check_against_reference(gw, R.reference(lg, c.prior, gt), f'V={V}: ')


def test_kernel_rejects_bad_arguments():
    V, images, K, l = 256, 2, 2, 3
    lg = torch.zeros(images * K * l, V, device='cuda'); gt = torch.zeros(images, l, dtype=torch.int64, device='cuda')
    prior = torch.full((images, K), 0.5, device='cuda'); ent = torch.zeros(images, K, l, device='cuda')
    o = [torch.zeros(images, l, device='cuda') for _ in range(4)]
    acc = (torch.zeros(images, l, V, dtype=torch.int64, device='cuda'), torch.zeros(images, l, dtype=torch.int64, device='cuda'),
           torch.zeros(images, l, dtype=torch.int32, device='cuda'))
    f, fin = hip.lib().fn['class_mix_f32'], hip.lib().fn['class_mix_finish_f32']
    st = hip.current_stream()
    p = lambda t: t.data_ptr()
    good = [p(lg), p(gt), l, images, K, l, V, 0, 1.0, 0.0, p(prior), K, p(ent), K * l, l, None, None, None, 0, p(o[0]), p(o[1]), p(o[2]), p(o[3]), l]
    assert f(*good, st) == 0
    torch.cuda.synchronize()
    assert float((o[2]).abs().max()) == 0.0 and float((ent - float(np.log(256))).abs().max()) < 1e-5       # equal rows: no information
    for pos, val in [(0, None), (1, None), (10, None), (12, None), (19, None), (20, None), (21, None), (22, None),
                     (2, l - 1), (11, K - 1), (14, l - 1), (13, K * l - 1), (23, l - 1),
                     (3, 0), (4, 0), (5, 0), (6, 0), (6, -4), (6, (1 << 24) + 1), (6, 4100)]:      # (V > 4096 has no on-chip route)
        a = list(good); a[pos] = val
        assert f(*a, st) == abi.EINVAL, (pos, val)
    chunk = list(good); chunk[15:24] = [p(acc[0]), p(acc[1]), p(acc[2]), l, None, None, None, None, 0]
    assert f(*chunk, st) == 0
    for pos, val in [(16, None), (17, None), (18, l - 1)]:
        a = list(chunk); a[pos] = val
        assert f(*a, st) == abi.EINVAL, (pos, val)
    goodf = [p(acc[0]), p(acc[1]), p(acc[2]), l, p(gt), l, images, l, V, p(o[0]), p(o[1]), p(o[2]), p(o[3]), l]
    assert fin(*goodf, st) == 0
    for pos, val in [(0, None), (1, None), (2, None), (4, None), (9, None), (10, None), (11, None), (12, None), (3, l - 1), (5, l - 1), (13, l - 1),
                     (6, 0), (7, 0), (8, 0), (8, (1 << 24) + 1)]:
        a = list(goodf); a[pos] = val
        assert fin(*a, st) == abi.EINVAL, (pos, val)
    torch.cuda.synchronize()


# ---- the model-level call -------------------------------------------------------------------------------------------
CLASSES = [1, 207, 999, 5, 417]
PERM = [3, 0, 4, 2, 1]
PRIOR = [0.3, 0.1, 0.25, 0.15, 0.2]


def fields(r):
    return dict(entropy=r.entropy, **{n: getattr(r, n) for n in OUT})


@pytest.mark.parametrize('prec', ['f32', 'bf16'])
@pytest.mark.parametrize('cfg', [0.0, 1.5])
def test_d16_against_float64_and_the_torch_route(prec, cfg):
    """var.class_information against the float64 restatement and class_information_torch, both applied to var(label, x)'s logits of the same
    precision.  Against float64: the twin-vs-float64 bounds.  Against the torch route (p and H rounded once from float64: inside the same
    bounds with room to spare): the sum of the two, twice the bound."""
    vae, var = d16()
    gt = tokens(var, 2, 11)
    with precision(var, prec), torch.no_grad():
        r = var.class_information(gt, CLASSES, cfg=cfg, prior=PRIOR)
        z = ref_rows(var, vae, gt, CLASSES, cfg)                       # (N, K, L, V)
    assert r.entropy.shape == (2, 5, var.L) and r.mi.shape == (2, var.L) and r.mi.is_cuda and r.patch_nums == tuple(var.patch_nums)
    pri = r.prior.cpu().numpy()
    Hpi = -float((pri[0].astype(np.float64) * np.log(pri[0].astype(np.float64))).sum())
    for i in range(2):
        for si, (b, e) in enumerate(var.begin_ends):
            got = {n: v[i:i + 1, ..., b:e].cpu().numpy() for n, v in fields(r).items()}
            ref = R.reference(z[i:i + 1, :, b:e].cpu().numpy(), pri[i:i + 1], gt[i:i + 1, b:e].cpu().numpy())
            R.check_against_reference(got, ref, f'{prec} cfg={cfg} image {i} scale {si} vs float64: ')
            assert (got['mi'] >= -ref['mi_bound']).all() and (got['mi'] <= Hpi + ref['mi_bound']).all(), '0 <= mi <= H(pi) up to the bound'
            t = class_information_torch(z[i, :, b:e], gt[i, b:e], r.prior[i])
            tor = dict(entropy=t[0].cpu().numpy()[None], **{n: v.cpu().numpy()[None] for n, v in zip(OUT, t[1:])})
            R.check_against_reference(tor, ref, f'{prec} cfg={cfg} image {i} scale {si} torch route vs float64: ')
            for n in ('entropy',) + OUT:
                d = np.abs(got[n].astype(np.float64) - tor[n].astype(np.float64))
                assert (d <= 2 * ref[R.BOUND_OF[n]]).all(), f'{prec} cfg={cfg} image {i} scale {si}: {n} differs from the torch route'
    ps = r.per_scale()
    assert ps['mi_mean'].shape == (2, len(var.patch_nums))
    assert r.mi_map(size=64).pred.shape == (2, 64, 64)


@pytest.mark.parametrize('prec', ['f32', 'bf16'])
def test_d16_bitwise_invariances_and_shared_workspace(prec):
    """integer sums: the (N, L) fields are the same bits across max_rows (6 and 3 force the chunked route), a permutation of the classes and a
    repeated call; token_log_likelihood around the call repeats bit for bit (one _tf_workspace for both)"""
    vae, var = d16()
    gt = tokens(var, 2, 13)
    classes = torch.tensor(CLASSES, device='cuda')
    perm = torch.tensor(PERM, device='cuda')
    prior = torch.tensor(PRIOR)
    with precision(var, prec):
        for cfg in (0.0, 1.5):
            lp0 = var.token_log_likelihood(gt, classes, cfg=cfg)
            base = var.class_information(gt, classes, cfg=cfg, max_rows=64, prior=prior)
            assert bool(torch.isfinite(base.mi).all())

            def same_tokens(r, what):
                for n in OUT:
                    assert torch.equal(getattr(r, n).view(torch.int32), getattr(base, n).view(torch.int32)), f'{prec} cfg={cfg} {what}: {n} differs'
            for mr in (64, 6, 3):
                r = var.class_information(gt, classes, cfg=cfg, max_rows=mr, prior=prior)
                same_tokens(r, f'max_rows={mr}')
                assert torch.equal(r.entropy.view(torch.int32), base.entropy.view(torch.int32)), f'{prec} cfg={cfg} max_rows={mr}: entropy differs'
            rp = var.class_information(gt, classes[perm], cfg=cfg, prior=prior[perm.cpu()])
            same_tokens(rp, 'permuted classes')
            assert torch.equal(rp.entropy.view(torch.int32), base.entropy[:, perm].view(torch.int32))
            assert torch.equal(var.token_log_likelihood(gt, classes, cfg=cfg), lp0), 'token_log_likelihood changed after class_information'


def test_d16_equal_labels_carry_no_information():
    vae, var = d16()
    gt = tokens(var, 2, 17)
    r = var.class_information(gt, [207] * 4, cfg=1.5)
    with torch.no_grad():
        z = ref_rows(var, vae, gt, [207] * 4, 1.5)
    for i in range(2):
        for b, e in var.begin_ends:
            ref = R.reference(z[i:i + 1, :, b:e].cpu().numpy(), r.prior[i:i + 1].cpu().numpy(), gt[i:i + 1, b:e].cpu().numpy())
            assert (np.abs(r.mi[i:i + 1, b:e].cpu().numpy()) <= ref['mi_bound']).all()
