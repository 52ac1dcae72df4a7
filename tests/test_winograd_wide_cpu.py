"""The host-side rule that picks the workgroup shape of varhip_conv3x3_wino_nhwc_f32 (varhip_wino_auto_shape, var_amd/csrc/winograd.hip):
host arithmetic, no GPU.  0 = 64 tiles x 32 channels (k_conv3x3_wino), 1 = the wide shape, 32 tiles x 80 channels (k_conv3x3_wino_wide)."""
import pytest

from var_amd import hip

# (H = W, Cin, Cout) of every fp32 decoder level at ch = 160 (tests/test_winograd_gpu.py::SHAPES) -> the shape DESIGN.md §13.3 records for it:
# the wide shape was 4-8 % faster at every one of them, 256^2 / 160 -> 160 included, so all six ship on it
RECORDED = {(256, 160, 160): 1, (128, 160, 160): 1, (64, 160, 320): 1, (64, 320, 320): 1, (32, 320, 320): 1, (16, 640, 640): 1}


@pytest.mark.parametrize('level', sorted(RECORDED))
def test_every_decoder_level_selects_the_recorded_shape(level):
    H, Cin, Cout = level
    assert Cout % 80 == 0
    assert hip.wino_auto_shape(H, H, Cin, Cout) == RECORDED[level]


def test_cout_no_multiple_of_80_never_selects_wide():
    so = hip.lib().so
    try:
        for force in (-1, 0, 1):
            hip.wino_force_shape(force)
            for Cout in (32, 64, 96, 128, 192, 224, 256, 288, 352, 608, 672):
                for H, Cin in ((16, 640), (64, 160), (256, 160)):
                    assert hip.wino_auto_shape(H, H, Cin, Cout) == 0
                    assert so.varhip_wino_pick_shape(H, H, Cin, Cout) == 0, (force, H, Cin, Cout)
        hip.wino_force_shape(1)
        assert so.varhip_wino_pick_shape(16, 16, 64, 80) == 1 and so.varhip_wino_pick_shape(16, 16, 64, 0) == 0
        hip.wino_force_shape(7)                                   # anything but 0 and 1 is "automatic"
        assert so.varhip_wino_pick_shape(16, 16, 64, 160) == hip.wino_auto_shape(16, 16, 64, 160)
    finally:
        hip.wino_force_shape(-1)
    assert hip.wino_last_shape() in (-1, 0, 1)
