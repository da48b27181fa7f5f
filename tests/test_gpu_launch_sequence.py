"""The ordered launches of one eager forward: every (label, flops, bytes) record rt.LaunchObserver takes
for the third call of a model (two warm-up calls first, as tools/trace_launches.py does) equals a
literal list.  The lists were recorded by running collect() of this file on the commit before the
layer executor was reorganised (one conv router, named records): a kernel re-routed, a launch
reordered, merged or split, or a changed work count shows up here as a changed list.
"""
import contextlib
import io

import pytest
import torch

import fastfourierconvolution_amd as F
from fastfourierconvolution_amd import _runtime as rt

pytestmark = pytest.mark.gpu
B = 4


def _gen64(train):
    return F.FFCGenerator(16, 3, 8).train(train), lambda m: m, (B, 16, 1, 1)


MODELS = {
    "gen_eval": lambda: _gen64(False),
    "gen_train": lambda: _gen64(True),
    "disc": lambda: (F.FFCDiscriminator(3, 8), lambda m: m, (B, 3, 64, 64)),
    "fgen32": lambda: (F.FGenerator32(128), lambda m: m.forward_float, (B, 128)),
}


def collect(name):
    """-> [(label, flops, bytes)] of one forward of MODELS[name] under no_grad, after two warm-up calls"""
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        model, fwd_of, shape = MODELS[name]()
    fwd = fwd_of(model.cuda())
    x = torch.randn(shape, device="cuda")
    obs = rt.LaunchObserver()
    with torch.no_grad():
        fwd(x)
        fwd(x)
        rt.set_observer(obs)
        try:
            fwd(x)
        finally:
            rt.set_observer(None)
    torch.cuda.synchronize()
    return [(label, float(work.get("flops", 0.0)), float(work.get("bytes", 0.0))) for label, _, _, work in obs.records]


EXPECTED = {
    "gen_eval": [
        ("dense", 131072.0, 0.0),
        ("st_prologue", 32768.0, 0.0),
        ("fu_pass1", 0.0, 12288.0),
        ("conv_gemm", 2473984.0, 0.0),
        ("st_prologue", 32768.0, 0.0),
        ("fu2d_r2c", 0.0, 9216.0),
        ("fu2d_mix1", 73728.0, 23552.0),
        ("fu2d_c2r", 0.0, 34816.0),
        ("conv_gemm", 2830336.0, 0.0),
        ("st_prologue", 32768.0, 0.0),
        ("fu2d_r2c", 0.0, 17408.0),
        ("fu2d_mix1", 69632.0, 44032.0),
        ("fu2d_c2r", 0.0, 67584.0),
        ("convt_smallm", 2097152.0, 0.0),
        ("conv_gemm", 1049600.0, 0.0),
        ("convt_smallm", 3145728.0, 0.0),
    ],
    "gen_train": [
        ("dense", 131072.0, 0.0),
        ("st_prologue", 32768.0, 0.0),
        ("fu_pass0", 0.0, 8192.0),
        ("fu_pass1", 0.0, 16384.0),
        ("conv_gemm", 2473984.0, 0.0),
        ("st_prologue", 32768.0, 0.0),
        ("bn_stats", 0.0, 0.0),
        ("fu2d_r2c", 0.0, 9216.0),
        ("fu2d_mix0", 73728.0, 23552.0),
        ("bn_stats", 0.0, 0.0),
        ("fu2d_c2r", 0.0, 34816.0),
        ("conv_gemm", 2830336.0, 0.0),
        ("st_prologue", 32768.0, 0.0),
        ("bn_stats", 0.0, 0.0),
        ("fu2d_r2c", 0.0, 17408.0),
        ("fu2d_mix0", 69632.0, 44032.0),
        ("bn_stats", 0.0, 0.0),
        ("fu2d_c2r", 0.0, 67584.0),
        ("convt_smallm", 2097152.0, 0.0),
        ("conv_gemm", 1049600.0, 0.0),
        ("convt_smallm", 3145728.0, 0.0),
    ],
    "disc": [
        ("conv_gemm", 6096384.0, 0.0),
        ("st_prologue", 131072.0, 0.0),
        ("bn_stats", 0.0, 0.0),
        ("fu2d_r2c", 0.0, 69632.0),
        ("fu2d_mix0", 294912.0, 73728.0),
        ("bn_stats", 0.0, 0.0),
        ("fu2d_c2r", 0.0, 69632.0),
        ("conv_gemm", 12070912.0, 0.0),
        ("st_prologue", 131072.0, 0.0),
        ("fu_pass0", 0.0, 16384.0),
        ("fu_pass1", 0.0, 32768.0),
        ("conv_gemm", 11321344.0, 0.0),
        ("st_prologue", 131072.0, 0.0),
        ("fu_pass0", 0.0, 8192.0),
        ("fu_pass1", 0.0, 16384.0),
        ("conv_gemm", 9895936.0, 0.0),
        ("conv_full_smallm", 16384.0, 0.0),
    ],
    "fgen32": [
        ("dense", 8388608.0, 0.0),
        ("conv_gemm", 205520896.0, 0.0),
        ("bn_stats", 0.0, 0.0),
        ("bn_act_noise", 0.0, 526336.0),
        ("st_prologue", 524288.0, 0.0),
        ("bn_stats", 0.0, 0.0),
        ("fu2d_r2c", 1179648.0, 90112.0),
        ("bn_stats", 0.0, 0.0),
        ("fu2d_c2r", 0.0, 139264.0),
        ("conv_gemm", 222232576.0, 0.0),
        ("bn_stats", 0.0, 0.0),
        ("bn_act_noise", 0.0, 1056768.0),
        ("st_prologue", 524288.0, 0.0),
        ("bn_stats", 0.0, 0.0),
        ("fu2d_r2c", 0.0, 69632.0),
        ("fu2d_mix0", 1114112.0, 176128.0),
        ("bn_stats", 0.0, 0.0),
        ("fu2d_c2r", 0.0, 270336.0),
        ("conv_gemm", 237223936.0, 0.0),
        ("bn_stats", 0.0, 0.0),
        ("conv3_smallm", 14155776.0, 0.0),
    ],
}


@pytest.mark.parametrize("name", list(MODELS))
def test_launch_sequence_is_the_recorded_one(name):
    got = collect(name)
    print(got)
    assert got == EXPECTED[name]
