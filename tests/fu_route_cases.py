"""Shared rows of tests/test_fu_route_cpu.py and tests/test_gpu_fu_route.py: one Fourier-unit call each, the
switches it runs under, the rt.FuRoute (and rt.st_conv1_route answer) expected for it, and in SEQUENCES the
ordered C entry points it launches.

The shapes are the smallest that take each branch of rt.fu_route: both sides of the fused kernel's fold
scratch (16 C H (W/2 + 1) >= 3072), of BN_FOLD_MAX (nrows C <= 4096), the split pass 1's channel rule, planes
only one path runs and planes both run, fp16, every staged switch, and bn1 folded, refused and demoted.

SEQUENCES was recorded with collect() of tests/test_gpu_fu_route.py at the commit before the router (see
that file); this module imports nothing of the package, so it loads there too.
"""
from typing import NamedTuple, Optional

ROUTE_DEFAULTS = dict(kgroups=1, spill=False, mix3=False, mix_fold=None, split_lanes=None, r2c_mix=False, mix1=None,
                      c2r=None, bn_kind=None)


def R(path, stats, in_fold, **kw):
    """the expected rt.FuRoute as a dict (rt.FuRoute._asdict())"""
    assert set(kw) <= set(ROUTE_DEFAULTS), kw
    return dict(path=path, stats=stats, in_fold=in_fold, **{**ROUTE_DEFAULTS, **kw})


class Row(NamedTuple):
    id: str
    kind: str                      # 'fu': FourierUnitSN._run(t, up=up) | 'st': SpectralTransform.spectral(x)
    B: int
    C: int                         # the Fourier unit's channels (st: out_channels // 2; in_channels = 16)
    H: int                         # the Fourier unit's (square) plane, after the st's pool / upsample
    up: int = 1                    # fu: up=; st: stride 2 with upsample
    pool: bool = False             # st: stride 2 without upsample (the input plane is 2H)
    train: bool = True
    mix: str = "fp32"
    lfu: bool = False              # st: run_lfu
    momentum_none: bool = False    # st: bn1.momentum = None
    sw: dict = {}                  # rt switches set for the row
    nrows: Optional[int] = None    # st: the rows of bn1's slab (conv1's statistics partials)
    conv1: Optional[str] = None    # st: the expected rt.st_conv1_route
    route: Optional[dict] = None   # the expected rt.FuRoute
    raises: Optional[str] = None   # a refusal: the start of the NotImplementedError's text


def _fused(in_fold=None, stats=True, **kw):
    kw.setdefault("spill", stats)
    return R("fused", stats, in_fold, **kw)


def _spilled(in_fold=None, **kw):          # staged, batch statistics, the Y spill
    kw.setdefault("c2r", "bn")
    return R("staged", True, in_fold, spill=True, **kw)


CH = {"BN_CHFOLD": True}
FUSED = {"FU_PATH": "fused"}
SLAB = dict(mix_fold="slab", bn_kind="slab")

ROWS = [
    # ---- the fused kernel's fold scratch, the split rule, mix3
    Row("fu_4x4_c4", "fu", 2, 4, 4, route=_fused()),
    Row("fu_8x8_c8", "fu", 2, 8, 8, route=_fused(mix3=True, split_lanes=4, **SLAB)),
    Row("fu_8x8_c8_chfold", "fu", 2, 8, 8, sw=CH,
        route=_fused(mix3=True, split_lanes=4, mix_fold="split", bn_kind="channels")),
    Row("fu_8x8_c8_chfold_nosplit", "fu", 2, 8, 8, sw={**CH, "FU_SPLIT": False}, route=_fused(mix3=True, **SLAB)),
    Row("fu_8x8_c8_nospill", "fu", 2, 8, 8, sw={"FU_SPILL": False}, route=_fused(mix3=True, spill=False, **SLAB)),
    Row("fu_8x8_c8_nofold", "fu", 2, 8, 8, sw={"BN_FOLD": False}, route=_fused(mix3=True, split_lanes=4)),
    Row("fu_8x8_c8_eval", "fu", 2, 8, 8, train=False, route=_fused(stats=False, mix3=True)),
    Row("fu_16_c4_fused", "fu", 2, 4, 16, sw=FUSED, route=_fused(split_lanes=8, **SLAB)),
    Row("fu_16_c4_fused_chfold", "fu", 2, 4, 16, sw={**FUSED, **CH},
        route=_fused(split_lanes=8, mix_fold="split", bn_kind="channels")),
    Row("fu_16_c6_fused_chfold", "fu", 2, 6, 16, sw={**FUSED, **CH}, route=_fused(**SLAB)),
    # ---- planes both paths run: the batch decides, FU_PATH and FORCE_FU2D override
    Row("fu_16_c8_B2", "fu", 2, 8, 16, route=_spilled()),
    Row("fu_16_c8_B2_fused", "fu", 2, 8, 16, sw=FUSED, route=_fused(mix3=True, split_lanes=8, **SLAB)),
    Row("fu_32_c8_B2", "fu", 2, 8, 32, route=_spilled()),
    Row("fu_32_c8_B2_fused", "fu", 2, 8, 32, sw=FUSED, route=_fused(mix3=True, split_lanes=16, **SLAB)),
    Row("fu_16_c8_B64", "fu", 64, 8, 16, route=_fused(mix3=True, split_lanes=8, **SLAB)),
    Row("fu_16_c8_B64_staged", "fu", 64, 8, 16, sw={"FU_PATH": "staged"}, route=_spilled()),
    Row("fu_16_c8_B64_force2d", "fu", 64, 8, 16, sw={"FORCE_FU2D": True}, route=_spilled()),
    Row("fu_16_c8_B2_minbatch", "fu", 2, 8, 16, sw={"FU_FUSED_MIN_BATCH": 2},
        route=_fused(mix3=True, split_lanes=8, **SLAB)),
    # ---- planes one path runs
    Row("fu_64_c8", "fu", 2, 8, 64, route=_spilled()),
    Row("fu_24_c8", "fu", 2, 8, 24, route=_fused(mix3=True, **SLAB)),
    Row("fu_48_up2_c8", "fu", 2, 8, 48, up=2, route=_fused(mix3=True, **SLAB)),
    # ---- fp16 mix, and the refusals
    Row("fu_32_c16_fp16", "fu", 2, 16, 32, mix="fp16", route=_spilled()),
    Row("fu_32_c16_fp16_eval", "fu", 2, 16, 32, mix="fp16", train=False, route=R("staged", False, None, mix1="cols",
                                                                                 c2r="rows")),
    Row("fu_32_c8_fp16_refused", "fu", 2, 8, 32, mix="fp16", raises="fp16 mix: staged FU with C in {16, 32, 64} only; "
                                                                    "got C=8, 32x32"),
    Row("fu_12_refused", "fu", 2, 8, 12, raises="Fourier unit supports H,W in {4,8,16,32}, square 24x24, or 48x48 as"),
    # ---- staged, batch statistics: spill x r2c_mix x channel fold
    Row("fu_16_c16", "fu", 2, 16, 16, route=_spilled(r2c_mix=True)),
    Row("fu_16_c16_ch", "fu", 2, 16, 16, sw=CH, route=_spilled(r2c_mix=True, c2r="fold", bn_kind="channels")),
    Row("fu_16_c16_nomix", "fu", 2, 16, 16, sw={"FU2D_R2CMIX": False}, route=_spilled()),
    Row("fu_16_c16_nomix_ch", "fu", 2, 16, 16, sw={"FU2D_R2CMIX": False, **CH},
        route=_spilled(c2r="fold", bn_kind="channels")),
    Row("fu_16_c16_nospill", "fu", 2, 16, 16, sw={"FU2D_SPILL": False},
        route=R("staged", True, None, mix1="plain", c2r="plain")),
    Row("fu_16_c16_nospill_ch", "fu", 2, 16, 16, sw={"FU2D_SPILL": False, **CH},
        route=R("staged", True, None, mix1="plain", c2r="plain")),
    Row("fu_16_c16_nospill_nomix", "fu", 2, 16, 16, sw={"FU2D_SPILL": False, "FU2D_R2CMIX": False},
        route=R("staged", True, None, mix1="plain", c2r="plain")),
    Row("fu_32_c16_nospill", "fu", 2, 16, 32, sw={"FU2D_SPILL": False},
        route=R("staged", True, None, mix1="cols", c2r="rows")),
    Row("fu_16_c16_ch_reads", "fu", 2, 16, 16, sw={**CH, "BN_CHFOLD_READS": 16}, route=_spilled(r2c_mix=True)),
    Row("fu_16_c16_ch_loads", "fu", 2, 16, 16, sw={**CH, "BN_CHFOLD_LOADS": 0}, route=_spilled(r2c_mix=True)),
    # ---- staged, running statistics: FU_COLS where the column kernel exists (H >= 32)
    Row("fu_32_c16_eval", "fu", 2, 16, 32, train=False, route=R("staged", False, None, mix1="cols", c2r="rows")),
    Row("fu_32_c16_eval_nocols", "fu", 2, 16, 32, train=False, sw={"FU_COLS": False},
        route=R("staged", False, None, mix1="plain", c2r="plain")),
    Row("fu_16_c16_eval", "fu", 2, 16, 16, train=False, route=R("staged", False, None, mix1="plain", c2r="plain")),
    Row("fu_16_c16_eval_nocols", "fu", 2, 16, 16, train=False, sw={"FU_COLS": False},
        route=R("staged", False, None, mix1="plain", c2r="plain")),
    # ---- bn1 in front of the unit (SpectralTransform), and conv1's kernel
    Row("st_8_c8", "st", 2, 8, 8, nrows=4, conv1="prologue", route=_fused("slab", mix3=True, split_lanes=4, **SLAB)),
    Row("st_4_c4", "st", 2, 4, 4, nrows=2, conv1="prologue", route=_fused()),
    Row("st_8_c8_eval", "st", 2, 8, 8, train=False, nrows=4, conv1="prologue", route=_fused(stats=False, mix3=True)),
    Row("st_8_c8_nofold", "st", 2, 8, 8, sw={"BN_FOLD": False}, nrows=4, conv1="prologue",
        route=_fused(mix3=True, split_lanes=4)),
    Row("st_8_c8_momentum_none", "st", 2, 8, 8, momentum_none=True, nrows=4, conv1="prologue",
        route=_fused("slab", mix3=True, split_lanes=4, **SLAB)),
    Row("st_8_c64_B64", "st", 64, 64, 8, sw={"ST_SPLIT": False}, nrows=64, conv1="prologue",
        route=_fused("slab", mix3=True, split_lanes=4)),
    Row("st_8_c64_B65", "st", 65, 64, 8, sw={"ST_SPLIT": False}, nrows=65, conv1="prologue",
        route=_fused(mix3=True, split_lanes=4)),
    Row("st_8_c64_B65_max", "st", 65, 64, 8, sw={"ST_SPLIT": False, "BN_FOLD_MAX": 65 * 128}, nrows=65,
        conv1="prologue", route=_fused("slab", mix3=True, split_lanes=4, **SLAB)),
    Row("st_8_c64_B65_ch", "st", 65, 64, 8, sw={"ST_SPLIT": False, **CH}, nrows=65, conv1="prologue",
        route=_fused(mix3=True, split_lanes=4)),   # the channel fold handed to a fused unit: its own launch
    Row("st_16_c16", "st", 2, 16, 16, nrows=8, conv1="prologue", route=_spilled(r2c_mix=True)),
    Row("st_16_c16_ch", "st", 2, 16, 16, sw=CH, nrows=8, conv1="prologue",
        route=_spilled("channels", r2c_mix=True, c2r="fold", bn_kind="channels")),
    Row("st_16_c16_ch_momentum_none", "st", 2, 16, 16, sw=CH, momentum_none=True, nrows=8, conv1="prologue",
        route=_spilled(r2c_mix=True, c2r="fold", bn_kind="channels")),
    Row("st_16_c16_ch_eval", "st", 2, 16, 16, sw=CH, train=False, nrows=8, conv1="prologue",
        route=R("staged", False, None, mix1="plain", c2r="plain")),
    Row("st_16_c8_lfu", "st", 2, 8, 16, lfu=True, nrows=8, conv1="prologue", route=_spilled()),
    Row("st_8_c8_lfu_fused", "st", 2, 8, 8, lfu=True, nrows=4, conv1="prologue",
        route=_fused(mix3=True, split_lanes=4, **SLAB)),
    Row("st_16_up2_c16", "st", 2, 16, 16, up=2, nrows=4, conv1="prologue", route=_spilled(r2c_mix=True)),
    Row("st_16_up2_c8_fused", "st", 2, 8, 16, up=2, sw=FUSED, nrows=4, conv1="prologue",
        route=_fused("slab", mix3=True, split_lanes=8, **SLAB)),
    Row("st_8_pool_c8", "st", 2, 8, 8, pool=True, nrows=4, conv1="prologue",
        route=_fused("slab", mix3=True, split_lanes=4, **SLAB)),
    Row("st_8_c8_pw", "st", 2, 8, 8, sw={"ST_PATH": "pw"}, nrows=2, conv1="pw_gate",
        route=_fused("slab", mix3=True, split_lanes=4, **SLAB)),
    Row("st_8_pool_c8_pw", "st", 2, 8, 8, pool=True, sw={"ST_PATH": "pw"}, nrows=4, conv1="gemm",
        route=_fused("slab", mix3=True, split_lanes=4, **SLAB)),
]
BY_ID = {r.id: r for r in ROWS}
assert len(BY_ID) == len(ROWS)

# (entry point -> positions of the arguments noted beside its name): the optional pointers, None or not, and
# the integer pass / kgroups
NOTED = {
    "ffc_fu_forward_ex4": dict(in_scale=6, in_shift=7, slab=12, scale=13, shift=14, in_fold=17, mix_fold=18,
                               yspill=19, **{"pass": 11, "kgroups": 20}),
    "ffc_fu2d_r2c_ex": dict(in_scale=5, in_shift=6, in_fold=8),
    "ffc_fu2d_r2c_mix": dict(in_scale=6, in_shift=7, in_fold=9, slab=11, yspill=12),
    "ffc_fu2d_mix": dict(slab=8, scale=9, shift=10, yspill=11, **{"pass": 7}),
    "ffc_fu2d_mix_f16": dict(slab=8, scale=9, shift=10, yspill=11, **{"pass": 7}),
}
# host-side queries (no launch): not part of a sequence
QUERY_SUFFIXES = ("_supported", "_elems", "_lds_bytes", "_kgroups", "_slab_rows", "_ws_doubles", "_blocks", "_prologue_split",
                  "_tiles", "_floats", "_version", "_last_error")


def note(name, args):
    """one recorded call: the entry point, then (for those in NOTED) pass / kgroups and the null pointers"""
    pos = NOTED.get(name)
    if pos is None:
        return name
    ints = [f"{k}={args[i]}" for k, i in pos.items() if k in ("pass", "kgroups")]
    nulls = [k for k, i in pos.items() if k not in ("pass", "kgroups") and args[i] is None]
    return f"{name}[{','.join(ints + ['null=' + '+'.join(nulls)])}]"


def implied(route, has_in_bn, f16=False):
    """the Fourier unit's own entry points (ffc_fu_forward* / ffc_fu2d_*) a route dict stands for, noted as
    note() does; has_in_bn: the call passes an input BN (st rows: folded, or as in_scale / in_shift)"""
    r = route
    aff = [] if has_in_bn else ["in_scale", "in_shift"]   # null when there is no input BN
    nofold = [] if r["in_fold"] else ["in_fold"]

    def fmt(name, ints, nulls):
        order = [k for k in NOTED[name] if k in nulls]
        return f"{name}[{','.join(ints + ['null=' + '+'.join(order)])}]"
    out = []
    if r["path"] == "fused":
        kg = f"kgroups={r['kgroups']}"
        spill = [] if r["spill"] else ["yspill"]
        if r["stats"]:
            out.append(fmt("ffc_fu_forward_ex4", ["pass=0", kg],
                           (["in_scale", "in_shift"] if r["in_fold"] else aff) + ["scale", "shift", "mix_fold"] +
                           nofold + spill))
        out.append(fmt("ffc_fu_forward_ex4", ["pass=1", kg],
                       aff + ["slab", "in_fold"] + (["scale", "shift"] if r["mix_fold"] else ["mix_fold"]) + spill))
        return out
    mix = "ffc_fu2d_mix_f16" if f16 else "ffc_fu2d_mix"
    if r["r2c_mix"]:
        out.append(fmt("ffc_fu2d_r2c_mix", [], (["in_scale", "in_shift"] if r["in_fold"] else aff) + nofold))
    else:
        out.append(fmt("ffc_fu2d_r2c_ex", [], (["in_scale", "in_shift"] if r["in_fold"] else aff) + nofold))
        if r["stats"]:
            out.append(fmt(mix, ["pass=0"], ["scale", "shift"] + ([] if r["spill"] else ["yspill"])))
    if r["mix1"] == "cols":
        out.append("ffc_fu2d_mix_cols")
    elif r["mix1"] == "plain":
        out.append(fmt(mix, ["pass=1"], ["slab"]))
    out.append("ffc_fu2d_c2r" + {"fold": "_fold", "bn": "_bn", "rows": "_rows", "plain": ""}[r["c2r"]])
    return out


# id -> the ordered entry points of the third call (two warm-up calls first), recorded before the router
SEQUENCES = {
    "fu_4x4_c4": [
        "ffc_fu_forward_ex4[pass=0,kgroups=1,null=in_scale+in_shift+scale+shift+in_fold+mix_fold]",
        "ffc_bn_reduce_finalize",
        "ffc_fu_forward_ex4[pass=1,kgroups=1,null=in_scale+in_shift+slab+in_fold+mix_fold]",
    ],
    "fu_8x8_c8": [
        "ffc_fu_forward_ex4[pass=0,kgroups=1,null=in_scale+in_shift+scale+shift+in_fold+mix_fold]",
        "ffc_fu_forward_ex4[pass=1,kgroups=1,null=in_scale+in_shift+slab+scale+shift+in_fold]",
    ],
    "fu_8x8_c8_chfold": [
        "ffc_fu_forward_ex4[pass=0,kgroups=1,null=in_scale+in_shift+scale+shift+in_fold+mix_fold]",
        "ffc_fu_forward_ex4[pass=1,kgroups=1,null=in_scale+in_shift+slab+scale+shift+in_fold]",
    ],
    "fu_8x8_c8_chfold_nosplit": [
        "ffc_fu_forward_ex4[pass=0,kgroups=1,null=in_scale+in_shift+scale+shift+in_fold+mix_fold]",
        "ffc_fu_forward_ex4[pass=1,kgroups=1,null=in_scale+in_shift+slab+scale+shift+in_fold]",
    ],
    "fu_8x8_c8_nospill": [
        "ffc_fu_forward_ex4[pass=0,kgroups=1,null=in_scale+in_shift+scale+shift+in_fold+mix_fold+yspill]",
        "ffc_fu_forward_ex4[pass=1,kgroups=1,null=in_scale+in_shift+slab+scale+shift+in_fold+yspill]",
    ],
    "fu_8x8_c8_nofold": [
        "ffc_fu_forward_ex4[pass=0,kgroups=1,null=in_scale+in_shift+scale+shift+in_fold+mix_fold]",
        "ffc_bn_reduce_finalize",
        "ffc_fu_forward_ex4[pass=1,kgroups=1,null=in_scale+in_shift+slab+in_fold+mix_fold]",
    ],
    "fu_8x8_c8_eval": [
        "ffc_bn_finalize",
        "ffc_fu_forward_ex4[pass=1,kgroups=1,null=in_scale+in_shift+slab+in_fold+mix_fold+yspill]",
    ],
    "fu_16_c4_fused": [
        "ffc_fu_forward_ex4[pass=0,kgroups=1,null=in_scale+in_shift+scale+shift+in_fold+mix_fold]",
        "ffc_fu_forward_ex4[pass=1,kgroups=1,null=in_scale+in_shift+slab+scale+shift+in_fold]",
    ],
    "fu_16_c4_fused_chfold": [
        "ffc_fu_forward_ex4[pass=0,kgroups=1,null=in_scale+in_shift+scale+shift+in_fold+mix_fold]",
        "ffc_fu_forward_ex4[pass=1,kgroups=1,null=in_scale+in_shift+slab+scale+shift+in_fold]",
    ],
    "fu_16_c6_fused_chfold": [
        "ffc_fu_forward_ex4[pass=0,kgroups=1,null=in_scale+in_shift+scale+shift+in_fold+mix_fold]",
        "ffc_fu_forward_ex4[pass=1,kgroups=1,null=in_scale+in_shift+slab+scale+shift+in_fold]",
    ],
    "fu_16_c8_B2": [
        "ffc_fu2d_r2c_ex[null=in_scale+in_shift+in_fold]",
        "ffc_fu2d_mix[pass=0,null=scale+shift]",
        "ffc_bn_reduce_finalize",
        "ffc_fu2d_c2r_bn",
    ],
    "fu_16_c8_B2_fused": [
        "ffc_fu_forward_ex4[pass=0,kgroups=1,null=in_scale+in_shift+scale+shift+in_fold+mix_fold]",
        "ffc_fu_forward_ex4[pass=1,kgroups=1,null=in_scale+in_shift+slab+scale+shift+in_fold]",
    ],
    "fu_32_c8_B2": [
        "ffc_fu2d_r2c_ex[null=in_scale+in_shift+in_fold]",
        "ffc_fu2d_mix[pass=0,null=scale+shift]",
        "ffc_bn_reduce_finalize",
        "ffc_fu2d_c2r_bn",
    ],
    "fu_32_c8_B2_fused": [
        "ffc_fu_forward_ex4[pass=0,kgroups=1,null=in_scale+in_shift+scale+shift+in_fold+mix_fold]",
        "ffc_fu_forward_ex4[pass=1,kgroups=1,null=in_scale+in_shift+slab+scale+shift+in_fold]",
    ],
    "fu_16_c8_B64": [
        "ffc_fu_forward_ex4[pass=0,kgroups=1,null=in_scale+in_shift+scale+shift+in_fold+mix_fold]",
        "ffc_fu_forward_ex4[pass=1,kgroups=1,null=in_scale+in_shift+slab+scale+shift+in_fold]",
    ],
    "fu_16_c8_B64_staged": [
        "ffc_fu2d_r2c_ex[null=in_scale+in_shift+in_fold]",
        "ffc_fu2d_mix[pass=0,null=scale+shift]",
        "ffc_bn_reduce_finalize",
        "ffc_fu2d_c2r_bn",
    ],
    "fu_16_c8_B64_force2d": [
        "ffc_fu2d_r2c_ex[null=in_scale+in_shift+in_fold]",
        "ffc_fu2d_mix[pass=0,null=scale+shift]",
        "ffc_bn_reduce_finalize",
        "ffc_fu2d_c2r_bn",
    ],
    "fu_16_c8_B2_minbatch": [
        "ffc_fu_forward_ex4[pass=0,kgroups=1,null=in_scale+in_shift+scale+shift+in_fold+mix_fold]",
        "ffc_fu_forward_ex4[pass=1,kgroups=1,null=in_scale+in_shift+slab+scale+shift+in_fold]",
    ],
    "fu_64_c8": [
        "ffc_fu2d_r2c_ex[null=in_scale+in_shift+in_fold]",
        "ffc_fu2d_mix[pass=0,null=scale+shift]",
        "ffc_bn_reduce_finalize",
        "ffc_fu2d_c2r_bn",
    ],
    "fu_24_c8": [
        "ffc_fu_forward_ex4[pass=0,kgroups=1,null=in_scale+in_shift+scale+shift+in_fold+mix_fold]",
        "ffc_fu_forward_ex4[pass=1,kgroups=1,null=in_scale+in_shift+slab+scale+shift+in_fold]",
    ],
    "fu_48_up2_c8": [
        "ffc_fu_forward_ex4[pass=0,kgroups=1,null=in_scale+in_shift+scale+shift+in_fold+mix_fold]",
        "ffc_fu_forward_ex4[pass=1,kgroups=1,null=in_scale+in_shift+slab+scale+shift+in_fold]",
    ],
    "fu_32_c16_fp16": [
        "ffc_fu2d_r2c_ex[null=in_scale+in_shift+in_fold]",
        "ffc_fu2d_mix_f16[pass=0,null=scale+shift]",
        "ffc_bn_reduce_finalize",
        "ffc_fu2d_c2r_bn",
    ],
    "fu_32_c16_fp16_eval": [
        "ffc_fu2d_r2c_ex[null=in_scale+in_shift+in_fold]",
        "ffc_bn_finalize",
        "ffc_fu2d_mix_cols",
        "ffc_fu2d_c2r_rows",
    ],
    "fu_16_c16": [
        "ffc_fu2d_r2c_mix[null=in_scale+in_shift+in_fold]",
        "ffc_bn_reduce_finalize",
        "ffc_fu2d_c2r_bn",
    ],
    "fu_16_c16_ch": [
        "ffc_fu2d_r2c_mix[null=in_scale+in_shift+in_fold]",
        "ffc_fu2d_c2r_fold",
    ],
    "fu_16_c16_nomix": [
        "ffc_fu2d_r2c_ex[null=in_scale+in_shift+in_fold]",
        "ffc_fu2d_mix[pass=0,null=scale+shift]",
        "ffc_bn_reduce_finalize",
        "ffc_fu2d_c2r_bn",
    ],
    "fu_16_c16_nomix_ch": [
        "ffc_fu2d_r2c_ex[null=in_scale+in_shift+in_fold]",
        "ffc_fu2d_mix[pass=0,null=scale+shift]",
        "ffc_fu2d_c2r_fold",
    ],
    "fu_16_c16_nospill": [
        "ffc_fu2d_r2c_ex[null=in_scale+in_shift+in_fold]",
        "ffc_fu2d_mix[pass=0,null=scale+shift+yspill]",
        "ffc_bn_reduce_finalize",
        "ffc_fu2d_mix[pass=1,null=slab]",
        "ffc_fu2d_c2r",
    ],
    "fu_16_c16_nospill_ch": [
        "ffc_fu2d_r2c_ex[null=in_scale+in_shift+in_fold]",
        "ffc_fu2d_mix[pass=0,null=scale+shift+yspill]",
        "ffc_bn_reduce_finalize",
        "ffc_fu2d_mix[pass=1,null=slab]",
        "ffc_fu2d_c2r",
    ],
    "fu_16_c16_nospill_nomix": [
        "ffc_fu2d_r2c_ex[null=in_scale+in_shift+in_fold]",
        "ffc_fu2d_mix[pass=0,null=scale+shift+yspill]",
        "ffc_bn_reduce_finalize",
        "ffc_fu2d_mix[pass=1,null=slab]",
        "ffc_fu2d_c2r",
    ],
    "fu_32_c16_nospill": [
        "ffc_fu2d_r2c_ex[null=in_scale+in_shift+in_fold]",
        "ffc_fu2d_mix[pass=0,null=scale+shift+yspill]",
        "ffc_bn_reduce_finalize",
        "ffc_fu2d_mix_cols",
        "ffc_fu2d_c2r_rows",
    ],
    "fu_16_c16_ch_reads": [
        "ffc_fu2d_r2c_mix[null=in_scale+in_shift+in_fold]",
        "ffc_bn_reduce_finalize",
        "ffc_fu2d_c2r_bn",
    ],
    "fu_16_c16_ch_loads": [
        "ffc_fu2d_r2c_mix[null=in_scale+in_shift+in_fold]",
        "ffc_bn_reduce_finalize",
        "ffc_fu2d_c2r_bn",
    ],
    "fu_32_c16_eval": [
        "ffc_fu2d_r2c_ex[null=in_scale+in_shift+in_fold]",
        "ffc_bn_finalize",
        "ffc_fu2d_mix_cols",
        "ffc_fu2d_c2r_rows",
    ],
    "fu_32_c16_eval_nocols": [
        "ffc_fu2d_r2c_ex[null=in_scale+in_shift+in_fold]",
        "ffc_bn_finalize",
        "ffc_fu2d_mix[pass=1,null=slab]",
        "ffc_fu2d_c2r",
    ],
    "fu_16_c16_eval": [
        "ffc_fu2d_r2c_ex[null=in_scale+in_shift+in_fold]",
        "ffc_bn_finalize",
        "ffc_fu2d_mix[pass=1,null=slab]",
        "ffc_fu2d_c2r",
    ],
    "fu_16_c16_eval_nocols": [
        "ffc_fu2d_r2c_ex[null=in_scale+in_shift+in_fold]",
        "ffc_bn_finalize",
        "ffc_fu2d_mix[pass=1,null=slab]",
        "ffc_fu2d_c2r",
    ],
    "st_8_c8": [
        "ffc_st_prologue_ex3",
        "ffc_fu_forward_ex4[pass=0,kgroups=1,null=in_scale+in_shift+scale+shift+mix_fold]",
        "ffc_fu_forward_ex4[pass=1,kgroups=1,null=slab+scale+shift+in_fold]",
    ],
    "st_4_c4": [
        "ffc_st_prologue_ex3",
        "ffc_bn_reduce_finalize",
        "ffc_fu_forward_ex4[pass=0,kgroups=1,null=scale+shift+in_fold+mix_fold]",
        "ffc_bn_reduce_finalize",
        "ffc_fu_forward_ex4[pass=1,kgroups=1,null=slab+in_fold+mix_fold]",
    ],
    "st_8_c8_eval": [
        "ffc_st_prologue_ex3",
        "ffc_bn_finalize",
        "ffc_bn_finalize",
        "ffc_fu_forward_ex4[pass=1,kgroups=1,null=slab+in_fold+mix_fold+yspill]",
    ],
    "st_8_c8_nofold": [
        "ffc_st_prologue_ex3",
        "ffc_bn_reduce_finalize",
        "ffc_fu_forward_ex4[pass=0,kgroups=1,null=scale+shift+in_fold+mix_fold]",
        "ffc_bn_reduce_finalize",
        "ffc_fu_forward_ex4[pass=1,kgroups=1,null=slab+in_fold+mix_fold]",
    ],
    "st_8_c8_momentum_none": [
        "ffc_st_prologue_ex3",
        "ffc_fu_forward_ex4[pass=0,kgroups=1,null=in_scale+in_shift+scale+shift+mix_fold]",
        "ffc_fu_forward_ex4[pass=1,kgroups=1,null=slab+scale+shift+in_fold]",
    ],
    "st_8_c64_B64": [
        "ffc_st_prologue_ex3",
        "ffc_fu_forward_ex4[pass=0,kgroups=1,null=in_scale+in_shift+scale+shift+mix_fold]",
        "ffc_bn_reduce_finalize",
        "ffc_fu_forward_ex4[pass=1,kgroups=1,null=slab+in_fold+mix_fold]",
    ],
    "st_8_c64_B65": [
        "ffc_st_prologue_ex3",
        "ffc_bn_reduce_finalize",
        "ffc_fu_forward_ex4[pass=0,kgroups=1,null=scale+shift+in_fold+mix_fold]",
        "ffc_bn_reduce_finalize",
        "ffc_fu_forward_ex4[pass=1,kgroups=1,null=slab+in_fold+mix_fold]",
    ],
    "st_8_c64_B65_max": [
        "ffc_st_prologue_ex3",
        "ffc_fu_forward_ex4[pass=0,kgroups=1,null=in_scale+in_shift+scale+shift+mix_fold]",
        "ffc_fu_forward_ex4[pass=1,kgroups=1,null=slab+scale+shift+in_fold]",
    ],
    "st_8_c64_B65_ch": [
        "ffc_st_prologue_ex3",
        "ffc_bn_reduce_finalize",
        "ffc_fu_forward_ex4[pass=0,kgroups=1,null=scale+shift+in_fold+mix_fold]",
        "ffc_bn_reduce_finalize",
        "ffc_fu_forward_ex4[pass=1,kgroups=1,null=slab+in_fold+mix_fold]",
    ],
    "st_16_c16": [
        "ffc_st_prologue_ex3",
        "ffc_bn_reduce_finalize",
        "ffc_fu2d_r2c_mix[null=in_fold]",
        "ffc_bn_reduce_finalize",
        "ffc_fu2d_c2r_bn",
    ],
    "st_16_c16_ch": [
        "ffc_st_prologue_ex3",
        "ffc_fu2d_r2c_mix[null=in_scale+in_shift]",
        "ffc_fu2d_c2r_fold",
    ],
    "st_16_c16_ch_momentum_none": [
        "ffc_st_prologue_ex3",
        "ffc_bn_reduce_finalize",
        "ffc_fu2d_r2c_mix[null=in_fold]",
        "ffc_fu2d_c2r_fold",
    ],
    "st_16_c16_ch_eval": [
        "ffc_st_prologue_ex3",
        "ffc_bn_finalize",
        "ffc_fu2d_r2c_ex[null=in_fold]",
        "ffc_bn_finalize",
        "ffc_fu2d_mix[pass=1,null=slab]",
        "ffc_fu2d_c2r",
    ],
    "st_16_c8_lfu": [
        "ffc_st_prologue_ex3",
        "ffc_bn_reduce_finalize",
        "ffc_lfu_gather",
        "ffc_fu_forward_ex4[pass=0,kgroups=1,null=in_scale+in_shift+scale+shift+in_fold+mix_fold]",
        "ffc_fu_forward_ex4[pass=1,kgroups=1,null=in_scale+in_shift+slab+scale+shift+in_fold]",
        "ffc_fu2d_r2c_ex[null=in_fold]",
        "ffc_fu2d_mix[pass=0,null=scale+shift]",
        "ffc_bn_reduce_finalize",
        "ffc_fu2d_c2r_bn",
        "ffc_lfu_tile_add",
    ],
    "st_8_c8_lfu_fused": [
        "ffc_st_prologue_ex3",
        "ffc_bn_reduce_finalize",
        "ffc_lfu_gather",
        "ffc_fu_forward_ex4[pass=0,kgroups=1,null=in_scale+in_shift+scale+shift+in_fold+mix_fold]",
        "ffc_bn_reduce_finalize",
        "ffc_fu_forward_ex4[pass=1,kgroups=1,null=in_scale+in_shift+slab+in_fold+mix_fold]",
        "ffc_fu_forward_ex4[pass=0,kgroups=1,null=scale+shift+in_fold+mix_fold]",
        "ffc_fu_forward_ex4[pass=1,kgroups=1,null=slab+scale+shift+in_fold]",
        "ffc_lfu_tile_add",
    ],
    "st_16_up2_c16": [
        "ffc_st_prologue_ex3",
        "ffc_bn_reduce_finalize",
        "ffc_fu2d_r2c_mix[null=in_fold]",
        "ffc_bn_reduce_finalize",
        "ffc_fu2d_c2r_bn",
    ],
    "st_16_up2_c8_fused": [
        "ffc_st_prologue_ex3",
        "ffc_fu_forward_ex4[pass=0,kgroups=1,null=in_scale+in_shift+scale+shift+mix_fold]",
        "ffc_fu_forward_ex4[pass=1,kgroups=1,null=slab+scale+shift+in_fold]",
    ],
    "st_8_pool_c8": [
        "ffc_st_prologue_ex3",
        "ffc_fu_forward_ex4[pass=0,kgroups=1,null=in_scale+in_shift+scale+shift+mix_fold]",
        "ffc_fu_forward_ex4[pass=1,kgroups=1,null=slab+scale+shift+in_fold]",
    ],
    "st_8_c8_pw": [
        "ffc_se_gate",
        "ffc_pw_gate_conv",
        "ffc_fu_forward_ex4[pass=0,kgroups=1,null=in_scale+in_shift+scale+shift+mix_fold]",
        "ffc_fu_forward_ex4[pass=1,kgroups=1,null=slab+scale+shift+in_fold]",
    ],
    "st_8_pool_c8_pw": [
        "ffc_se_gate",
        "ffc_conv_forward",
        "ffc_fu_forward_ex4[pass=0,kgroups=1,null=in_scale+in_shift+scale+shift+mix_fold]",
        "ffc_fu_forward_ex4[pass=1,kgroups=1,null=slab+scale+shift+in_fold]",
    ],
}
