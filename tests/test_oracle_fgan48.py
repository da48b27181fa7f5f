"""Pins the oracle compositions of the 8*mg family (tests/fgan48_refs.py) against the reference's own
fp64 outputs at mg = 6 (tests/golden/gen_golden_fgan48.py), in the style of test_oracle_golden.py: the
GPU machine then never needs the reference.  Fixtures are stored as float32, hence the 1e-6 bound."""
import json
import os

import numpy as np
import pytest
import torch

import fgan48_refs as R
from conftest import GOLDEN
from fixture_weights import input_array, make_state
from oracle.ffc_oracle import normwise_err, quantize_u8

with open(os.path.join(GOLDEN, "manifest_fgan48.json")) as _f:
    MANIFEST = json.load(_f)
CASES = {c["name"]: c for c in MANIFEST["cases"]}


def _load(name):
    c = CASES[name]
    data = np.load(os.path.join(GOLDEN, name + ".npz"))
    state = make_state(c["seed"], c["specs"])
    for k in data.files:
        if k.startswith("before."):
            state[k[len("before."):]] = data[k]
    sd = {k: torch.from_numpy(np.array(v)) for k, v in state.items()}
    sd = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    tin = {k: torch.from_numpy(input_array(c["seed"], k, shp)).double() for k, shp in c["inputs"].items()}
    return c, sd, tin, data


def test_oracle_generator_train():
    c, sd, tin, data = _load("fgan48_gen_train")
    noises = [(tin[f"noise{n}_l"], tin[f"noise{n}_g"]) for n in (2, 3, 4)]
    out = R.fgan32_generator(tin["z"], sd, True, noises, mg=6)
    assert tuple(out.shape) == (2, 3, 48, 48)
    assert normwise_err(out, torch.from_numpy(data["ref.out"])) < 1e-6


def test_oracle_generator_eval():
    c, sd, tin, data = _load("fgan48_gen_eval")
    out = R.fgan32_generator(tin["z"], sd, False, mg=6)
    assert normwise_err(out, torch.from_numpy(data["ref.out"])) < 1e-6
    assert torch.equal(quantize_u8(out.clamp(-1, 1)), torch.from_numpy(data["ref.out_u8"]))


@pytest.mark.parametrize("name,fn", [("fgan48_disc", R.fgan32_discriminator), ("fgan48_fdisc", R.fgan32_fdiscriminator)])
def test_oracle_critics(name, fn):
    c, sd, tin, data = _load(name)
    out = fn(tin["x"], sd, True, mg=6)
    assert normwise_err(out, torch.from_numpy(data["ref.out"])) < 1e-6
    for k in data.files:
        if k.startswith("after.") and k.endswith(("weight_u", "weight_v")):
            assert normwise_err(sd[k[len("after."):]], torch.from_numpy(data[k])) < 1e-6, k
