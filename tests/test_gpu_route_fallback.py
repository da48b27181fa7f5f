"""Eval forwards of layers at and just over the channel caps of the small-M and dense kernels
(rt.RouteCaps): at the cap the direct kernel runs, over it the job falls back to the implicit-GEMM
kernels.  Both against torch.nn.functional in float64 on the CPU at the project's gate, normwise
(max|a - ref| / max|ref|) <= 1e-4.
"""
import contextlib
import io

import pytest
import torch
import torch.nn.functional as TF

import fastfourierconvolution_amd as F
from fastfourierconvolution_amd import _runtime as rt
from oracle.ffc_oracle import normwise_err

pytestmark = pytest.mark.gpu
B = 2

CASES = {   # name: (layer constructor, input plane, fp64 reference, label of the direct kernel)
    "convT": (lambda C: F.FFCTranspose(C, 3, 4, 0, 0, stride=2, padding=1), 4,
              lambda x, w: TF.conv_transpose2d(x, w, stride=2, padding=1), "convt_smallm"),
    "conv3": (lambda C: F.FFC(C, 3, 3, 0, 0, stride=1, padding=1), 8,
              lambda x, w: TF.conv2d(x, w, stride=1, padding=1), "conv3_smallm"),
    "dense": (lambda C: F.FFCTranspose(C, 8, 4, 0, 0), 1,
              lambda x, w: TF.conv_transpose2d(x, w), "dense"),
}


@pytest.mark.parametrize("C,direct", [(256, True), (260, False)], ids=["at_cap", "over_cap"])
@pytest.mark.parametrize("name", list(CASES))
def test_eval_forward_at_and_over_the_cap(name, C, direct):
    make, side, ref_fn, label = CASES[name]
    torch.manual_seed(3)
    with contextlib.redirect_stdout(io.StringIO()):
        layer = make(C).eval()
    x = torch.randn(B, C, side, side)
    ref = ref_fn(x.double(), layer.convl2l.weight.detach().double())
    layer = layer.cuda()
    obs = rt.LaunchObserver()
    rt.set_observer(obs)
    try:
        with torch.no_grad():
            out_l, out_g = layer(x.cuda())
    finally:
        rt.set_observer(None)
    torch.cuda.synchronize()
    labels = [r[0] for r in obs.records]
    err = normwise_err(out_l.cpu(), ref)
    print(name, C, labels, f"normwise {err:.3e}")
    assert labels == [label if direct else "conv_gemm"]
    assert isinstance(out_g, int) and out_g == 0
    assert tuple(out_l.shape) == tuple(ref.shape) and err <= 1e-4
