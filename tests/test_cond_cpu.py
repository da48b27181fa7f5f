"""Class-conditional fgan128 without a GPU: the state_dict of FCondGenerator / FCondDiscriminator is the
reference's (keys and shapes of tests/golden/manifest_cond.json, loaded strictly), the two new ops'
meta functions give the right shapes and dtypes, the C ABI still reports version 4, and the
distributed wrappers refuse the conditional models."""
import contextlib
import io
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from fixture_weights import make_state


def _cases():
    with open(os.path.join(GOLDEN, "manifest_cond.json")) as f:
        return json.load(f)["cases"]


def _build(case):
    import fastfourierconvolution_amd as F
    with contextlib.redirect_stdout(io.StringIO()):
        return getattr(F, case["kind"])(**case["ctor"])


@pytest.mark.parametrize("case", _cases(), ids=lambda c: c["name"])
def test_state_dict_is_the_references(case):
    mod = _build(case)
    sd = mod.state_dict()
    assert set(sd) == set(case["specs"])
    for k, spec in case["specs"].items():
        assert list(sd[k].shape) == list(spec[0]), k
    state = make_state(case["seed"], case["specs"])
    mod.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in state.items()}, strict=True)


def test_default_constructors_and_key_families():
    import fastfourierconvolution_amd as F
    with contextlib.redirect_stdout(io.StringIO()):
        G = F.FCondGenerator(128)
    D = F.FCondDiscriminator()
    assert G.ngf == 64 and G.num_classes == 10 and tuple(G.label_embed.weight.shape) == (10, 10)
    assert tuple(G.input_conv[0].weight.shape) == (128, 256, 4, 4)
    assert tuple(G.label_conv[0].weight.shape) == (10, 256, 4, 4)
    tops = {k.split(".")[0] for k in G.state_dict()}
    want = {f"conv{n}" for n in range(2, 8)} | {f"{b}_noise{n}" for b in ("lcl", "glb") for n in range(2, 7)} | \
        {"label_conv", "input_conv", "label_embed"}
    assert tops == want
    assert tuple(D.conv1.weight_orig.shape) == (64, 4, 3, 3) and tuple(D.label_embed.weight.shape) == (10, 128 * 128)
    assert {k.split(".")[0] for k in D.state_dict()} == {f"conv{n}" for n in range(1, 10)} | {"fc", "label_embed"}
    assert isinstance(G, F.FGenerator)   # the trunk, noises, forward_float and the uint8 head are FGenerator's


def test_meta_functions():
    B, K, NC = 3, 100, 10
    m = lambda *s, **k: torch.empty(*s, device="meta", **k)   # noqa: E731
    labels = m(B, dtype=torch.int64)
    args = (m(B, K), labels, m(NC, NC), m(K, 256, 4, 4), m(256), m(NC, 256, 4, 4), m(256), m(256), m(256), m(256),
            m(256), m(256), m(256), m(256), m(256))
    for use_batch in (True, False):
        y, pre, scale, shift, stats = torch.ops.ffc.cond_stem(*args, use_batch, 1e-5)
        assert tuple(y.shape) == tuple(pre.shape) == (B, 512, 4, 4) and y.dtype == torch.float32
        assert tuple(scale.shape) == tuple(shift.shape) == (512,)
        if use_batch:
            assert tuple(stats.shape) == (512, 3) and stats.dtype == torch.float64
        else:
            assert tuple(stats.shape) == (2, 512) and stats.dtype == torch.float32
    outs = torch.ops.ffc.cond_stem_backward(m(B, 512, 4, 4), m(B, K), labels, m(NC, NC), m(K, 256, 4, 4),
                                            m(NC, 256, 4, 4), [False, True, True, True, True, False])
    assert [tuple(t.shape) for t in outs] == [(0,), (NC, NC), (K, 256, 4, 4), (256,), (NC, 256, 4, 4), (0,)]
    plane = torch.ops.ffc.embed_rows(m(NC, 16384), labels)
    assert tuple(plane.shape) == (B, 16384) and plane.dtype == torch.float32
    g = torch.ops.ffc.embed_rows_backward(m(B, 16384), labels, NC)
    assert tuple(g.shape) == (NC, 16384) and g.dtype == torch.float32


def test_abi_version_unchanged_and_entry_points_bound():
    from fastfourierconvolution_amd import _lib
    lib = _lib.load()
    assert lib.ffc_abi_version() == 4
    assert lib.ffc_cond_stem_slab_rows(1) == 1 and lib.ffc_cond_stem_slab_rows(33) == 2
    assert lib.ffc_cond_stem_forward(None, None, None, None, None, None, None, 1, 8, 3, None, None, None) == -1
    assert b"ffc_cond_stem_forward" in lib.ffc_last_error()
    assert lib.ffc_embed_gather_rows(None, None, 1, 3, 16, None, None) == -1
    assert lib.ffc_embed_scatter_rows(None, None, 1, 3, 16, None, None) == -1


def test_product_path_refuses_cpu_labels_and_tensors():
    import fastfourierconvolution_amd as F
    from fastfourierconvolution_amd import _lib
    with contextlib.redirect_stdout(io.StringIO()):
        G = F.FCondGenerator(8, num_classes=3)
    with pytest.raises(_lib.FFCError, match="no CPU fallback"):
        G(torch.randn(2, 8), torch.tensor([0, 1]))


def test_distributed_wrappers_refuse_the_conditional_models():
    import fastfourierconvolution_amd as F
    from fastfourierconvolution_amd import distributed as dist_
    with contextlib.redirect_stdout(io.StringIO()):
        G = F.FCondGenerator(8, num_classes=3)
    D = F.FCondDiscriminator(num_classes=3)
    for m in (G, D, torch.nn.Sequential(D)):
        with pytest.raises(NotImplementedError, match="conditional"):
            dist_.broadcast_module(m)
        with pytest.raises(NotImplementedError, match="conditional"):
            dist_.refuse_conditional(m)
    dist_.refuse_conditional(F.Discriminator())   # the unconditional models are untouched
