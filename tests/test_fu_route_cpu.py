"""rt.fu_route and rt.st_conv1_route, the one place that decides which kernels run a Fourier unit and who
finalizes which BatchNorm, and rt.bn_fold_kind, the fold predicate under them: pure functions of shapes,
BN facts, the switches of _runtime and the library's host-side queries (the library loads without a device).

The rows of tests/fu_route_cases.py carry the expected records as literals; tests/test_gpu_fu_route.py ties
the same rows to what is launched.
"""
import pytest
import torch

from fastfourierconvolution_amd import _runtime as rt
from fu_route_cases import ROWS, Row

# the switches of rt.PLAN_KNOBS the two routers and the predicate read
READ = ("FORCE_FU2D", "FU_PATH", "FU_FUSED_MIN_BATCH", "FU_COLS", "FU2D_SPILL", "BN_FOLD", "BN_FOLD_MAX", "FU_SPILL",
        "ST_PATH", "BN_CHFOLD", "BN_CHFOLD_LOADS", "BN_CHFOLD_READS", "FU2D_R2CMIX", "FU_SPLIT", "FU_KGROUPS",
        "BN_FOLD_SYNC")


def answer(row: Row):
    """-> (the FuRoute as a dict, or the refusal's text; st_conv1_route or None) under the current switches"""
    conv1 = in_bn = None
    if row.kind == "st":
        h = row.H * 2 if row.pool else row.H // row.up
        conv1 = rt.st_conv1_route(row.B, 16, h, h, row.pool, 1, row.C)   # SELayer(16): one hidden unit
        in_bn = rt.InBn(row.nrows, float(row.up * row.up), row.train, row.momentum_none, row.lfu)
    try:
        return rt.fu_route(row.B, row.C, row.H, row.H, row.up, row.mix, row.train, False, in_bn)._asdict(), conv1
    except NotImplementedError as e:
        return str(e), conv1


@pytest.mark.parametrize("row", ROWS, ids=[r.id for r in ROWS])
def test_route_table(row, monkeypatch):
    for k, v in row.sw.items():
        monkeypatch.setattr(rt, k, v)
    got, conv1 = answer(row)
    assert conv1 == row.conv1
    if row.raises is not None:
        assert isinstance(got, str) and got.startswith(row.raises)
    else:
        assert got == row.route


def test_routers_allocate_and_launch_nothing(monkeypatch):
    """every row again with torch.empty and every entry point but the host-side queries made to raise"""
    queries = ("ffc_fu_supported", "ffc_fu2d_supported", "ffc_fu_mix3_elems", "ffc_fu_kgroups", "ffc_fu_slab_rows",
               "ffc_fu2d_slab_rows", "ffc_fu2d_r2c_mix_supported", "ffc_fu2d_cols_supported",
               "ffc_st_prologue_lds_bytes", "ffc_pw_gate_lds_bytes")
    real = rt.lib()

    class QueriesOnly:
        def __getattr__(self, name):
            assert name in queries, f"{name} reached from a router"
            return getattr(real, name)

    def no_alloc(*a, **k):
        raise AssertionError("torch.empty reached from a router")
    monkeypatch.setattr(rt, "lib", lambda: QueriesOnly())
    monkeypatch.setattr(torch, "empty", no_alloc)
    for row in ROWS:
        with monkeypatch.context() as m:
            for k, v in row.sw.items():
                m.setattr(rt, k, v)
            got, _ = answer(row)
            assert got == row.route or got.startswith(row.raises)


# (BN_FOLD_SYNC, momentum is None, lanes) -> bn_fold_kind under a sync group
SYNC = [
    (True, False, None, "moments"),
    (True, True, None, "moments"),      # the whole-slab rule never looked at the momentum
    (True, False, 64, "moments"),
    (True, True, 64, None),             # per channel: the leaders cannot read num_batches_tracked
    (False, False, None, None),
    (False, False, 64, None),
]


@pytest.mark.parametrize("sync_on,momentum_none,lanes,want", SYNC)
def test_fold_predicate_under_a_sync_group(sync_on, momentum_none, lanes, want, monkeypatch):
    monkeypatch.setattr(rt, "_sync_group", lambda: object())
    monkeypatch.setattr(rt, "BN_FOLD_SYNC", sync_on)
    monkeypatch.setattr(rt, "BN_CHFOLD", True)
    # no row gating on moments: far over every single-rank limit
    assert rt.bn_fold_kind(10 ** 6, 512, True, momentum_none, lanes=lanes, consumers=10 ** 6) == want
    assert rt.bn_fold_kind(8, 8, False, momentum_none, lanes=lanes) is None   # running statistics never fold
    monkeypatch.setattr(rt, "BN_CHFOLD", False)
    assert rt.bn_fold_kind(8, 8, True, momentum_none, lanes=lanes) == (want if lanes is None else None)


def test_routes_under_a_sync_group(monkeypatch):
    """SyncBN: bn1 as a moments fold on both paths (per channel on the staged one, so not without a momentum),
    and the unit's own BN from the merged moments wherever a single rank folds it"""
    monkeypatch.setattr(rt, "_sync_group", lambda: object())
    bn1 = rt.InBn(8, 1.0, True, False)
    r = rt.fu_route(2, 8, 8, 8, 1, "fp32", True, False, bn1)
    assert (r.path, r.in_fold, r.mix_fold, r.bn_kind) == ("fused", "moments", "slab", "moments")
    r = rt.fu_route(2, 4, 4, 4, 1, "fp32", True, False, bn1)     # no fold scratch in the planes: moments need none
    assert (r.in_fold, r.mix_fold) == ("moments", None)
    r = rt.fu_route(2, 16, 16, 16, 1, "fp32", True, False, bn1)
    assert (r.path, r.in_fold, r.c2r) == ("staged", "moments", "bn")   # BN_CHFOLD is off: the C2R does not fold
    assert rt.fu_route(2, 16, 16, 16, 1, "fp32", True, False, bn1._replace(momentum_none=True)).in_fold is None
    assert rt.fu_route(2, 8, 8, 8, 1, "fp32", True, False, bn1._replace(consumers_other=True)).in_fold is None
    monkeypatch.setattr(rt, "BN_FOLD_SYNC", False)
    r = rt.fu_route(2, 8, 8, 8, 1, "fp32", True, False, bn1)
    assert (r.in_fold, r.mix_fold) == (None, None)


def test_a_ready_descriptor_keeps_its_kind():
    """FourierUnitSN._run(in_fold=): the caller's descriptor is taken as made (no second look at BN_FOLD_MAX)
    where the path folds that kind, asked again per channel on the staged path, its own launch otherwise"""
    big = rt.InBn(10 ** 6, 1.0, True, False, ready="slab")
    assert rt.fu_route(2, 8, 8, 8, 1, "fp32", True, False, big).in_fold == "slab"
    assert rt.fu_route(2, 4, 4, 4, 1, "fp32", True, False, big).in_fold is None            # no fold scratch
    assert rt.fu_route(2, 8, 8, 8, 1, "fp32", False, False, big).in_fold is None           # no pass 0 in eval mode
    assert rt.fu_route(2, 8, 8, 8, 1, "fp32", True, False, big._replace(ready="channels")).in_fold is None
    assert rt.fu_route(2, 16, 16, 16, 1, "fp32", True, False, big._replace(nrows=8)).in_fold is None   # BN_CHFOLD off


@pytest.mark.parametrize("knob", READ)
def test_every_switch_read_changes_an_answer(knob, monkeypatch):
    """a switch that is read nowhere would leave every answer as it was"""
    assert knob in rt.PLAN_KNOBS
    flipped = {"FU_PATH": "fused", "ST_PATH": "pw", "FU_FUSED_MIN_BATCH": 1, "BN_FOLD_MAX": 8, "BN_CHFOLD_LOADS": 0,
               "BN_CHFOLD_READS": 1}
    value = flipped.get(knob, not getattr(rt, knob))

    def table():
        out = [answer(r) for r in ROWS if knob not in r.sw]
        # FU_KGROUPS gates a library answer that is off without FFC_FU_KGROUPS=2, and BN_FOLD_SYNC needs a
        # sync group: asked with stand-ins for both
        with monkeypatch.context() as m:
            real = rt.lib()

            class TwoGroups:
                def __getattr__(self, name):
                    return (lambda *a: 2) if name == "ffc_fu_kgroups" else getattr(real, name)
            m.setattr(rt, "lib", lambda: TwoGroups())
            out.append(rt.fu_route(64, 8, 16, 16, 1, "fp32", True, False).kgroups)
            m.setattr(rt, "_sync_group", lambda: object())
            out.append(rt.bn_fold_kind(8, 8, True, False))
        return out
    with monkeypatch.context() as m:   # the channel-fold limits show only with the fold on
        m.setattr(rt, "BN_CHFOLD", True) if knob.startswith("BN_CHFOLD_") else None
        before = table()
        m.setattr(rt, knob, value)
        assert table() != before
