"""VAR.autoregressive_infer_cfg_with_mask without a GPU: argument checks (ValueError before the device check), the CPU model's RuntimeError,
models.var.get_edit_mask against hand-written boxes, the reference fixtures' self-consistency (tools/gen_golden_edit.py), and the new C ABI
entries (their table, the Makefile, the notebook cell the header cites)."""
import contextlib
import io
import json
import os

import numpy as np
import pytest
import torch

from models import build_vae_var
from models.var import get_edit_mask
from var_amd.detinit import fill_module_

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PNS = (1, 2, 3, 4, 5)
L = sum(p * p for p in PNS)
_M = {}


def cpu_model():
    if 'm' not in _M:
        with contextlib.redirect_stdout(io.StringIO()):
            vae, var = build_vae_var(device='cpu', patch_nums=PNS, depth=2, ch=32)
        fill_module_(var, 2, 0, 'var.'); fill_module_(vae, 2, 0, 'vae.')
        _M['m'] = (vae.eval(), var.eval())
    return _M['m']


def good(B=2):
    toks = [torch.randint(0, 4096, (B, p * p)) for p in PNS]
    return dict(B=B, label_B=3, input_img_tokens=toks, edit_mask=torch.ones(5, 5))


def test_method_exists():
    from models import VAR
    assert callable(getattr(VAR, 'autoregressive_infer_cfg_with_mask', None))


BAD = [
    dict(edit_mask=None),                                                     # one of the two only
    dict(input_img_tokens=None),
    dict(B=0),
    dict(B=2.0),
    dict(input_img_tokens=[torch.zeros(2, p * p, dtype=torch.long) for p in PNS[:-1]]),        # a scale missing
    dict(input_img_tokens=[torch.zeros(2, p * p + 1, dtype=torch.long) for p in PNS]),         # wrong scale length
    dict(input_img_tokens=[torch.zeros(2, p * p, dtype=torch.float32) for p in PNS]),          # not integer
    dict(input_img_tokens=[torch.zeros(2, p * p, dtype=torch.bool) for p in PNS]),
    dict(input_img_tokens=[torch.full((2, p * p), 4096, dtype=torch.long) for p in PNS]),      # out of range
    dict(input_img_tokens=[torch.full((2, p * p), -1, dtype=torch.long) for p in PNS]),
    dict(input_img_tokens=torch.zeros(3, L, dtype=torch.long)),                                # rows neither 1 nor B
    dict(input_img_tokens=torch.zeros(2, L - 1, dtype=torch.long)),
    dict(input_img_tokens=torch.zeros(2, L, 1, dtype=torch.long)),
    dict(input_img_tokens=np.zeros((2, L), np.int64)),
    dict(edit_mask=torch.ones(5)),                                                             # mask shapes
    dict(edit_mask=torch.ones(1, 1, 5, 5)),
    dict(edit_mask=torch.ones(3, 5, 5)),
    dict(edit_mask=torch.ones(0, 5)),
    dict(edit_mask=torch.ones(5, 0)),
    dict(edit_mask=torch.ones(5, 5, dtype=torch.complex64)),
    dict(edit_mask=np.ones((5, 5), np.float32)),
    dict(label_B=torch.tensor([1.0, 2.0])),
    dict(label_B=torch.tensor([1, 2, 3])),
]


@pytest.mark.parametrize('i', range(len(BAD)))
def test_malformed_arguments_raise_value_error_before_the_device_check(i):
    _, var = cpu_model()
    kw = good()
    kw.update(BAD[i])
    with pytest.raises(ValueError):
        var.autoregressive_infer_cfg_with_mask(**kw)


@pytest.mark.parametrize('variant', ['list', 'concat', 'one_row', 'bool_mask', 'batched_mask', 'int_mask', 'odd_mask', 'more_smooth'])
def test_well_formed_call_raises_the_no_fallback_runtime_error(variant):
    _, var = cpu_model()
    kw = good(3)
    if variant == 'concat': kw['input_img_tokens'] = torch.cat(kw['input_img_tokens'], 1)
    if variant == 'one_row': kw['input_img_tokens'] = [t[:1] for t in kw['input_img_tokens']]
    if variant == 'bool_mask': kw['edit_mask'] = torch.rand(5, 5) < 0.5
    if variant == 'batched_mask': kw['edit_mask'] = torch.rand(3, 7, 9)
    if variant == 'int_mask': kw['edit_mask'] = torch.ones(1, 16, 16, dtype=torch.int32)
    if variant == 'odd_mask': kw['edit_mask'] = torch.ones(1, 1, dtype=torch.float64)
    if variant == 'more_smooth': kw['more_smooth'] = True
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        var.autoregressive_infer_cfg_with_mask(**kw)


def test_without_mask_is_plain_sampling():
    _, var = cpu_model()
    with pytest.raises(RuntimeError, match='VAR.autoregressive_infer_cfg:'):
        var.autoregressive_infer_cfg_with_mask(2, 3, g_seed=0)


def box(P, r0, r1, c0, c1, inpainting):
    m = np.zeros((P, P), np.float32)
    m[r0:r1, c0:c1] = 1
    return 1 - m if inpainting else m


@pytest.mark.parametrize('inpainting', [True, False])
def test_get_edit_mask_matches_hand_written_boxes(inpainting):
    # Python round (half to even): 0.1 * 16 = 1.6 -> 2, 0.8 * 16 = 12.8 -> 13; 0.5 * 5 = 2.5 -> 2, 0.3 * 5 = 1.5 -> 2
    cases = [((1, 2, 3, 4, 5, 6, 8, 10, 13, 16), (0.1, 0.1, 0.8, 0.8), (2, 13, 2, 13)),
             ((1, 2, 3, 4, 5), (0.5, 0.3, 0.9, 1.0), (2, 4, 2, 5)),
             ((1, 2, 3, 4, 6, 9, 13, 18, 24, 32), (0.0, 0.25, 0.75, 0.5), (0, 24, 8, 16)),
             ((1, 2, 3, 4, 5), (0.0, 0.0, 1.0, 1.0), (0, 5, 0, 5))]
    for pns, (y0, x0, y1, x1), (r0, r1, c0, c1) in cases:
        m = get_edit_mask(pns, y0, x0, y1, x1, 'cpu', inpainting=inpainting)
        assert m.dtype == torch.float32 and tuple(m.shape) == (pns[-1],) * 2
        assert np.array_equal(m.numpy(), box(pns[-1], r0, r1, c0, c1, inpainting)), (pns, y0, x0, y1, x1)


def test_get_edit_mask_is_exported_by_models_var():
    import models.var as mv
    assert mv.get_edit_mask is get_edit_mask


EDIT_FIXTURES = ['a_inpaint', 'b_outpaint', 'c_b3_7x9', 'd_more_smooth', 'e_saln', 'f_half']


@pytest.mark.parametrize('name', EDIT_FIXTURES)
def test_fixture_keep_maps_follow_the_rule_and_final_tokens_the_mask(name, golden_dir):
    """the recorded keep maps equal F.interpolate(mask) > 0.5 on this CPU (pn^2 <= 3 kept whole), and final = where(keep, input, sampled)"""
    import torch.nn.functional as F
    z = np.load(f'{golden_dir}/edit_{name}.npz')
    meta = json.loads(str(z['meta']))
    B, pns = meta['B'], meta['patch_nums']
    mask = torch.from_numpy(z['mask'])
    mask = mask.expand(B, -1, -1) if mask.shape[0] == 1 else mask
    want = []
    for pn in pns:
        k = F.interpolate(mask[:, None], size=(pn, pn), mode='bilinear', align_corners=False) > 0.5
        if pn * pn <= 3: k[:] = True
        want.append(k.view(B, -1))
    want = torch.cat(want, 1).numpy()
    assert np.array_equal(z['keep'].astype(bool), want)
    assert np.array_equal(z['final'], np.where(z['keep'].astype(bool), z['tokens'], z['sampled']))
    assert z['f_hat'].shape == (B, 32, pns[-1], pns[-1]) and z['img'].shape == (B, 3, 16 * pns[-1], 16 * pns[-1])


def test_lambda_half_fixture_exercises_the_edge(golden_dir):
    """case f reads its 0/1 edge at a source coordinate of 7.5 + 1 ulp (pn = 13): the recorded map is what the fused rounding gives"""
    z = np.load(f'{golden_dir}/edit_f_half.npz')
    meta = json.loads(str(z['meta']))
    pns = meta['patch_nums']
    si = pns.index(13)
    b0 = sum(p * p for p in pns[:si])
    k13 = z['keep'][0, b0:b0 + 169].reshape(13, 13)
    assert k13[6, 0] == 1 and k13[0, 6] == 1 and k13[5, 5] == 0


def test_new_entry_points_in_header_and_abi_with_matching_argument_lists():
    """(the argument lists themselves: tests/test_abi_cpu.py, for every declaration of the header)"""
    from var_amd import abi
    header = open(os.path.join(ROOT, 'include', 'var_hip.h')).read()
    for name in ('edit_keep_u8', 'quant_accum_edit_f32', 'quant_accum_h_edit_f32'):
        assert name in abi.SIGNATURES_HIP_ONLY, name
    assert 'edit.hip' in open(os.path.join(ROOT, 'var_amd', 'csrc', 'Makefile')).read().split('SRCS16')[0]
    assert 'demo_zero_shot_edit.ipynb cell 2' in header
