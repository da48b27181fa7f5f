"""The case table, float64 references and fixed-seed input builders of the convq kernel
(csrc/convq_kernels.hip: ffc_convq_forward / ffc_convq_forward_split), shared by test_convq_cases_cpu.py
(the table against the planner, the references against torch.nn.functional; no GPU) and
test_gpu_convq_kernels.py (the kernel against the references).

A case is (B, M, segments) plus, per cfg it runs under, the plan facts it is there for, written out as
literals: FACTS[name][cfg] = (NS, TR, TC, nrb, ncb, staging width).  The facts are restated here, not read
from the planner: test_convq_cases_cpu.py fails when plan_convq_job and this table disagree, and when the
sets of branches the table reaches (coverage()) differ from the written-out lists there.

Host rules restated (csrc/convq_kernels.hip):
  chunks        a segment has Cpad / 16 = ceil(C / 16) chunks of K; the staged segments' chunks come first (job
                order), then the direct (1x1) segments'
  units4        max over the staged segments of the launch's jobs of 2 NS PR (PC / 4): staging units of four
                pixels x eight channels per chunk, at most 256 (CONVQ_MAX_UNITS)
  staging width stage_px: units4 <= 64 -> 1 pixel per unit, <= 128 -> 2, else 4; cfg 0..2 have no 1-pixel
                kernel and run width 1 on the 2 variant
  K split       split ks of n takes chunks [lo, hi) = [ntot ks / n, ntot (ks + 1) / n) (integer division) of that
                sequence: slo = min(lo, nstaged), nst = min(hi, nstaged) - slo staged chunks, then the direct
                chunks [max(lo, nstaged), max(hi, nstaged)) - nstaged
  tiles         one per (pixel block, 32 MT output channels) and split: npb ceil(M / (32 MT)) ksplit rows,
                npb = ceil(B / NS) nrb ncb"""
import collections

import numpy as np
import torch

import conv_refs as cr
from fastfourierconvolution_amd import _plan

CFGS = {0: (1, 4), 1: (1, 2), 2: (2, 2), 3: (1, 1)}   # cfg -> (MT, NTW), ffc_convq_config
MAX_UNITS = 256

Case = collections.namedtuple("Case", "B M segs")


def T(C, H, W, op=0):
    """ConvTranspose2d k4 s2 p1 (output_padding op) on C x H x W: a staged segment"""
    return ("convT", C, H, W, 4, 2, 1, 1, op)


def P(C, H, W):
    """1x1 at the output resolution H x W: a direct segment"""
    return ("pw", C, H, W)


def segs_of(case):
    return [_plan.Seg(*s) for s in case.segs]


def _one(H, W, C=9, B=3, M=40):
    return Case(B, M, (T(C, H, W),))


CASES = {
    # ---- chunk pipeline: 4x4 inputs, B 3, M 40
    "ch1": _one(4, 4, 7), "ch2": _one(4, 4, 20), "ch3": _one(4, 4, 33), "ch4": _one(4, 4, 64),
    "ch5": _one(4, 4, 80), "ch7": _one(4, 4, 100),
    "seg2x1": Case(3, 40, (T(16, 4, 4), T(9, 4, 4))),
    "st3d1": Case(3, 40, (T(40, 4, 4), P(16, 8, 8))),
    "stdrag": Case(3, 40, (T(20, 4, 4), P(5, 8, 8))),
    "ct3seg": Case(3, 40, (T(20, 4, 4), T(12, 4, 4), P(8, 8, 8))),
    # ---- geometry
    "g1x4": _one(1, 4), "g2x8": _one(2, 8), "g3x4": _one(3, 4), "g4x12": _one(4, 12), "g5x20": _one(5, 20),
    "g12x4": _one(12, 4), "g9x28": _one(9, 28),
    "w68": Case(1, 40, (T(9, 2, 68), P(5, 4, 136))), "w132": Case(1, 40, (T(9, 1, 132),)),
    "h24w8": _one(24, 8, B=1), "h22w8": _one(22, 8, B=1),
    "b5": _one(4, 4, B=5), "b7": _one(4, 4, B=7), "b11": _one(2, 8, B=11),
    # output_padding 1: the phases differ in size (PH = IH + 1 / IH), and the last row block holds pixels of
    # the py = 0 phases only: waves 2 and 3 of that block have no valid pixel (slab rows {0, 0, 0})
    "op12": Case(1, 40, (T(9, 12, 4, 1),)), "op25": Case(1, 40, (T(9, 25, 4, 1),)),
    # ---- epilogue
    "m1": _one(4, 4, 20, M=1), "m31": _one(4, 4, 20, M=31), "m32": _one(4, 4, 20, M=32),
    "m33": _one(4, 4, 20, M=33), "m64": _one(4, 4, 20, M=64), "m70": _one(4, 4, 20, M=70),
    "m130": _one(4, 4, 20, M=130),
    "full70": Case(2, 70, (T(16, 8, 8),)),       # every pixel block full: the unmasked store path, and M-tile 64.. masked
    # ---- second job of the two-job launches (beside ct3seg)
    "ct33": Case(2, 33, (T(33, 8, 8),)),
    # ---- K split: 2 + 2 staged chunks, 2 direct chunks (157 real k: the integer builder stays exact)
    "ks6": Case(3, 40, (T(17, 4, 4), T(18, 4, 4), P(17, 8, 8))),
    "ks33": Case(3, 40, (T(33, 4, 4), P(40, 8, 8))),   # 3 staged + 3 direct chunks
    # ---- persistent loop: more tiles than 4 workgroups on each of 256 CUs, per cfg
    "pers0": Case(1645, 130, (T(24, 2, 8),)), "pers1": Case(826, 130, (T(24, 2, 8),)),
    "pers2": Case(1372, 130, (T(24, 2, 8),)), "pers3": Case(413, 130, (T(24, 2, 8),)),
}
PERSIST = {0: "pers0", 1: "pers1", 2: "pers2", 3: "pers3"}
PERSIST_DISTINCT = 7       # distinct samples of a persistent case's batch (sample b is sample b % 7)
PERSIST_BOUND = 4 * 256    # tiles a case must exceed: 4 resident 512-thread workgroups on each of 256 CUs

# FACTS[name][cfg] = (NS, TR, TC, nrb, ncb, staging width); a case runs under exactly the cfgs listed
FACTS = {
    "ch1": {0: (3, 4, 4, 1, 1, 2), 1: (3, 4, 4, 1, 1, 2), 2: (3, 4, 4, 1, 1, 2), 3: (2, 4, 4, 1, 1, 2)},
    "ch2": {0: (3, 4, 4, 1, 1, 2), 1: (3, 4, 4, 1, 1, 2), 2: (3, 4, 4, 1, 1, 2), 3: (2, 4, 4, 1, 1, 2)},
    "ch3": {0: (3, 4, 4, 1, 1, 2), 1: (3, 4, 4, 1, 1, 2), 2: (3, 4, 4, 1, 1, 2), 3: (2, 4, 4, 1, 1, 2)},
    "ch4": {0: (3, 4, 4, 1, 1, 2), 1: (3, 4, 4, 1, 1, 2), 2: (3, 4, 4, 1, 1, 2), 3: (2, 4, 4, 1, 1, 2)},
    "ch5": {0: (3, 4, 4, 1, 1, 2), 1: (3, 4, 4, 1, 1, 2), 2: (3, 4, 4, 1, 1, 2), 3: (2, 4, 4, 1, 1, 2)},
    "ch7": {0: (3, 4, 4, 1, 1, 2), 1: (3, 4, 4, 1, 1, 2), 2: (3, 4, 4, 1, 1, 2), 3: (2, 4, 4, 1, 1, 2)},
    "seg2x1": {0: (3, 4, 4, 1, 1, 2), 1: (3, 4, 4, 1, 1, 2), 2: (3, 4, 4, 1, 1, 2), 3: (2, 4, 4, 1, 1, 2)},
    "st3d1": {0: (3, 4, 4, 1, 1, 2), 1: (3, 4, 4, 1, 1, 2), 2: (3, 4, 4, 1, 1, 2), 3: (2, 4, 4, 1, 1, 2)},
    "stdrag": {0: (3, 4, 4, 1, 1, 2), 1: (3, 4, 4, 1, 1, 2), 2: (3, 4, 4, 1, 1, 2), 3: (2, 4, 4, 1, 1, 2)},
    "ct3seg": {0: (3, 4, 4, 1, 1, 2), 1: (3, 4, 4, 1, 1, 2), 2: (3, 4, 4, 1, 1, 2), 3: (2, 4, 4, 1, 1, 2)},
    "g1x4": {0: (3, 1, 4, 1, 1, 2), 1: (3, 1, 4, 1, 1, 2), 2: (3, 1, 4, 1, 1, 2), 3: (3, 1, 4, 1, 1, 1)},
    "g2x8": {0: (3, 2, 8, 1, 1, 2), 1: (3, 2, 8, 1, 1, 2), 2: (3, 2, 8, 1, 1, 2), 3: (2, 2, 8, 1, 1, 1)},
    "g3x4": {0: (3, 3, 4, 1, 1, 2), 1: (3, 3, 4, 1, 1, 2), 2: (3, 3, 4, 1, 1, 2), 3: (2, 3, 4, 1, 1, 1)},
    "g4x12": {0: (2, 4, 12, 1, 1, 2), 1: (1, 4, 12, 1, 1, 2), 2: (1, 4, 12, 1, 1, 2), 3: (1, 2, 12, 2, 1, 1)},
    "g5x20": {0: (1, 5, 20, 1, 1, 2), 1: (1, 3, 20, 2, 1, 2), 2: (1, 3, 20, 2, 1, 2), 3: (1, 1, 20, 5, 1, 1)},
    "g12x4": {0: (2, 12, 4, 1, 1, 4), 1: (1, 12, 4, 1, 1, 2), 2: (1, 12, 4, 1, 1, 2), 3: (1, 8, 4, 2, 1, 1)},
    "g9x28": {0: (1, 4, 28, 3, 1, 2), 1: (1, 2, 28, 5, 1, 2), 2: (1, 2, 28, 5, 1, 2), 3: (1, 1, 28, 9, 1, 1)},
    "w68": {0: (1, 1, 68, 2, 1, 2), 1: (1, 1, 64, 2, 2, 2), 2: (1, 1, 64, 2, 2, 2), 3: (1, 1, 32, 2, 3, 1)},
    "w132": {0: (1, 1, 128, 1, 2, 2), 1: (1, 1, 64, 1, 3, 2), 2: (1, 1, 64, 1, 3, 2), 3: (1, 1, 32, 1, 5, 1)},
    "h24w8": {0: (1, 16, 8, 2, 1, 4), 1: (1, 8, 8, 3, 1, 2), 2: (1, 8, 8, 3, 1, 2), 3: (1, 4, 8, 6, 1, 1)},
    "h22w8": {0: (1, 16, 8, 2, 1, 4), 1: (1, 8, 8, 3, 1, 2), 2: (1, 8, 8, 3, 1, 2), 3: (1, 4, 8, 6, 1, 1)},
    "b5": {0: (5, 4, 4, 1, 1, 4), 1: (4, 4, 4, 1, 1, 4), 2: (4, 4, 4, 1, 1, 4), 3: (2, 4, 4, 1, 1, 2)},
    "b7": {0: (7, 4, 4, 1, 1, 4), 1: (4, 4, 4, 1, 1, 4), 2: (4, 4, 4, 1, 1, 4), 3: (2, 4, 4, 1, 1, 2)},
    "b11": {0: (8, 2, 8, 1, 1, 4), 1: (4, 2, 8, 1, 1, 2), 2: (4, 2, 8, 1, 1, 2), 3: (2, 2, 8, 1, 1, 1)},
    "op12": {0: (1, 13, 5, 1, 1, 2), 1: (1, 12, 5, 2, 1, 2), 2: (1, 12, 5, 2, 1, 2), 3: (1, 6, 5, 3, 1, 1)},
    "op25": {0: (1, 25, 5, 2, 1, 4), 1: (1, 12, 5, 3, 1, 2), 2: (1, 12, 5, 3, 1, 2), 3: (1, 6, 5, 5, 1, 1)},
    "m1": {0: (3, 4, 4, 1, 1, 2), 1: (3, 4, 4, 1, 1, 2), 2: (3, 4, 4, 1, 1, 2), 3: (2, 4, 4, 1, 1, 2)},
    "m31": {0: (3, 4, 4, 1, 1, 2), 1: (3, 4, 4, 1, 1, 2), 2: (3, 4, 4, 1, 1, 2), 3: (2, 4, 4, 1, 1, 2)},
    "m32": {0: (3, 4, 4, 1, 1, 2), 1: (3, 4, 4, 1, 1, 2), 2: (3, 4, 4, 1, 1, 2), 3: (2, 4, 4, 1, 1, 2)},
    "m33": {0: (3, 4, 4, 1, 1, 2), 1: (3, 4, 4, 1, 1, 2), 2: (3, 4, 4, 1, 1, 2), 3: (2, 4, 4, 1, 1, 2)},
    "m64": {0: (3, 4, 4, 1, 1, 2), 1: (3, 4, 4, 1, 1, 2), 2: (3, 4, 4, 1, 1, 2), 3: (2, 4, 4, 1, 1, 2)},
    "m70": {0: (3, 4, 4, 1, 1, 2), 1: (3, 4, 4, 1, 1, 2), 2: (3, 4, 4, 1, 1, 2), 3: (2, 4, 4, 1, 1, 2)},
    "m130": {0: (3, 4, 4, 1, 1, 2), 1: (3, 4, 4, 1, 1, 2), 2: (3, 4, 4, 1, 1, 2), 3: (2, 4, 4, 1, 1, 2)},
    "full70": {0: (2, 8, 8, 1, 1, 4), 1: (1, 8, 8, 1, 1, 2), 2: (1, 8, 8, 1, 1, 2), 3: (1, 4, 8, 2, 1, 1)},
    "ct33": {0: (2, 8, 8, 1, 1, 4), 1: (1, 8, 8, 1, 1, 2), 2: (1, 8, 8, 1, 1, 2), 3: (1, 4, 8, 2, 1, 1)},
    "ks6": {0: (3, 4, 4, 1, 1, 2), 1: (3, 4, 4, 1, 1, 2), 2: (3, 4, 4, 1, 1, 2), 3: (2, 4, 4, 1, 1, 2)},
    "ks33": {0: (3, 4, 4, 1, 1, 2), 1: (3, 4, 4, 1, 1, 2), 2: (3, 4, 4, 1, 1, 2), 3: (2, 4, 4, 1, 1, 2)},
    "pers0": {0: (8, 2, 8, 1, 1, 4)},
    "pers1": {1: (4, 2, 8, 1, 1, 2)},
    "pers2": {2: (4, 2, 8, 1, 1, 2)},
    "pers3": {3: (2, 2, 8, 1, 1, 1)},
}

# launches of more than one case: name -> (cases, cfgs, expected staging width per cfg)
PAIRS = {"pair": (("ct3seg", "ct33"), (0, 1, 2, 3))}
PAIR_WIDTH = {"pair": {0: 4, 1: 2, 2: 2, 3: 2}}   # units4 is the launch's maximum: 160 (ct33) / 108 / 108 / 72 (ct3seg)

# K split: (case, forced ksplit) -> [(staged chunks, direct chunks) per split] (min(forced, chunks) splits)
KSPLITS = {
    ("ks6", 2): [(3, 0), (1, 2)],                      # split 1 starts at chunk 1 of the second staged segment
    ("ks6", 3): [(2, 0), (2, 0), (0, 2)],              # staged only, starting in a later segment, direct only
    ("ks6", 4): [(1, 0), (2, 0), (1, 0), (0, 2)],      # split 1 crosses the segment change
    ("ks6", 8): [(1, 0)] * 4 + [(0, 1)] * 2,           # min(8, 6 chunks) splits
    ("ks33", 2): [(3, 0), (0, 3)],
    ("ks33", 4): [(1, 0), (2, 0), (0, 1), (0, 2)],     # the last split starts at direct chunk 1
    ("ct3seg", 3): [(1, 0), (1, 0), (1, 1)],           # 4 chunks: 4 k / 3 = 0, 1, 2, 4
}

# shapes that must not plan: name -> (B, M, segments, reason)
NO_PLAN = {
    "iw6": (3, 40, (T(9, 5, 6),), "staged IW % 4 != 0"),
    "pooled": (2, 40, (T(9, 4, 4), ("pw", 6, 8, 8, 1, 1, 0, 1, 0, True, False)), "a pooled segment"),
    "gated": (2, 40, (T(9, 4, 4), ("pw", 6, 8, 8, 1, 1, 0, 1, 0, False, True)), "a gated segment"),
    "units": (8, 40, (T(9, 4, 4),), "cfg 0: NS 8, 2 * 8 * 6 * 3 = 288 units > CONVQ_MAX_UNITS"),
    "k6s2": (2, 40, (("convT", 9, 4, 4, 6, 2, 2),), "ConvT k6 s2 p2: 9 taps per phase"),
    "k3s1": (2, 40, (("convT", 9, 4, 4, 3, 1, 1),), "ConvT k3 s1 p1: one phase"),
    "k4s4": (2, 40, (("convT", 9, 4, 4, 4, 4, 0),), "ConvT k4 s4: 16 phases"),
    "conv3": (2, 40, (("conv", 9, 4, 4, 3, 1, 1),), "Conv2d k3: one phase"),
    "pwonly": (2, 40, (P(9, 8, 8),), "1x1 alone: one phase, not at twice a phase grid"),
}
NO_PLAN_CFGS = {"units": (0,)}   # default: every cfg


# --------------------------------------------------------------------------- the host rules, restated
def chunks(case):
    """16-channel chunks per segment"""
    return tuple(-(-s[1] // 16) for s in case.segs)


def staged_direct(case):
    """(chunks of the staged segments in job order, total direct chunks)"""
    ch = chunks(case)
    return [c for c, s in zip(ch, case.segs) if s[0] != "pw"], sum(c for c, s in zip(ch, case.segs) if s[0] == "pw")


def patch_shape(TR, TC, IH):
    """(PR, PC) of a ConvT k4 s2 p1 segment's patch: phase-grid pixels step one input pixel, the four phases'
    taps span offsets -1 .. 1 (a one-row input keeps offset 0 only: the other taps never meet it), and a row
    is staged in 4-pixel groups from its start rounded down to a multiple of 4 (up to 3 columns more)"""
    return TR + (2 if IH > 1 else 0), 4 * ((TC + 2 + 6) // 4)


def units4(case, facts):
    NS, TR, TC = facts[:3]
    PR, PC = patch_shape(TR, TC, case.segs[0][2])
    return 2 * NS * PR * (PC // 4) if any(s[0] != "pw" for s in case.segs) else 0


def stage_width(cfg, u4):
    fit = 1 if u4 <= 64 else 2 if u4 <= 128 else 4
    return fit if cfg == 3 else max(fit, 2)


def split_ranges(case, ksplit):
    """[(staged chunks, direct chunks)] per split, and per split where its first staged chunk lies:
    (staged segment index, chunk inside it) or None"""
    st, nd = staged_direct(case)
    nstaged, ntot = sum(st), sum(st) + nd
    out, starts = [], []
    for ks in range(ksplit):
        lo, hi = ntot * ks // ksplit, ntot * (ks + 1) // ksplit
        slo = min(lo, nstaged)
        nst = min(hi, nstaged) - slo
        dlo, dhi = max(lo, nstaged) - nstaged, max(hi, nstaged) - nstaged
        out.append((nst, dhi - dlo))
        s, c = 0, slo
        while nst and c >= st[s]:
            c -= st[s]
            s += 1
        starts.append((s, c) if nst else None)
    return out, starts


def split_kinds(case, ksplit):
    """the kinds of split a K-split launch of the case contains"""
    kinds = set()
    for (nst, nd), start in zip(*split_ranges(case, ksplit)):
        kinds.add("staged only" if nst and not nd else "direct only" if nd and not nst else "both")
        if start is not None and start[1] > 0:
            kinds.add("starts mid-segment")
        if start is not None and start[0] > 0:
            kinds.add("starts in a later segment")
    return kinds


def ntiles(case, cfg, facts, ksplit=1):
    NS, TR, TC, nrb, ncb = facts[:5]
    return -(-case.B // NS) * nrb * ncb * -(-case.M // (32 * CFGS[cfg][0])) * ksplit


def coverage():
    """the branch sets the table reaches, from the written-out facts alone"""
    cov = collections.defaultdict(set)
    for name, per in FACTS.items():
        c = CASES[name]
        st, nd = staged_direct(c)
        for cfg, f in per.items():
            NS, TR, TC, nrb, ncb, width = f
            cov["cfg_width"].add((cfg, width))
            if ntiles(c, cfg, f) > PERSIST_BOUND:
                cov["cfg_persistent"].add(cfg)
            cov["nst"].add((sum(st) % 2, sum(st)))
            for key, hit in (("nrb>1", nrb > 1), ("ncb>1", ncb > 1), ("ragged B % NS", c.B % NS != 0),
                             ("ragged rows", (c.segs[0][2] + c.segs[0][8] if c.segs[0][0] == "convT" else 0) % TR != 0),
                             ("NS*TR*TC < 32*NTW", NS * TR * TC < 32 * CFGS[cfg][1]),
                             ("NS*TR*TC == 32*NTW", NS * TR * TC == 32 * CFGS[cfg][1]),
                             ("C < 8", any(s[1] < 8 and s[0] != "pw" for s in c.segs)),
                             ("C % 16 != 0", any(s[1] % 16 for s in c.segs)),
                             ("direct C % 16 != 0", any(s[1] % 16 and s[0] == "pw" for s in c.segs))):
                if hit:
                    cov[key].add(cfg)
    for (name, ks) in KSPLITS:
        cov["split_kinds"] |= split_kinds(CASES[name], min(ks, sum(chunks(CASES[name]))))
        for nst, _ in split_ranges(CASES[name], min(ks, sum(chunks(CASES[name]))))[0]:
            cov["nst"].add((nst % 2, nst))
    for names, cfgs in PAIRS.values():
        cov["njobs=2"] |= set(cfgs)
    return dict(cov)


# --------------------------------------------------------------------------- references
def abs_sum_ref(segs, d):
    """S[b, m, y, x] = sum |w| |x| + |bias| + |addend|: the same job on the absolute values (float64)"""
    ab = lambda t: None if t is None else t.double().abs()   # noqa: E731
    pre, _ = cr.conv_job_ref(segs, [ab(x) for x in d["xs"]], [ab(w) for w in d["ws"]], d["layouts"], None,
                             ab(d["bias"]), ab(d["addend"]))
    return pre


def job_ref(segs, d, act=0):
    """(pre, out) in float64 of a builder's inputs"""
    return cr.conv_job_ref(segs, d["xs"], d["ws"], d["layouts"], None, d["bias"], d["addend"], act, cr.SLOPE)


def slab_ref(pre):
    """the merged {n, mean, M2} per channel of the pre-activation output (float64)"""
    n, mean, var = cr.channel_stats(pre)
    return n, mean, var * n


def slab_row_counts(case, facts):
    """valid pixels of every slab row [pixel block * 4 + phase]: the count column of the slab, exactly"""
    NS, TR, TC, nrb, ncb = facts[:5]
    sg = case.segs[0]
    OH, OW = 2 * sg[2] + sg[8], 2 * sg[3] + sg[8]
    rows = []
    for bs in range(-(-case.B // NS)):
        for rb in range(nrb):
            for cb in range(ncb):
                for py in (0, 1):
                    for px in (0, 1):
                        PH, PW = -(-(OH - py) // 2), -(-(OW - px) // 2)
                        rows.append(min(NS, case.B - bs * NS) * max(0, min(TR, PH - rb * TR)) * max(0, min(TC, PW - cb * TC)))
    return torch.tensor(rows, dtype=torch.float64)


# --------------------------------------------------------------------------- input builders
def _shapes(B, M, segs):
    xs = [(B, sg.C, sg.IH, sg.IW) for sg in segs]
    ws = [(sg.C, M, 4, 4) if sg.kind == "convT" else (M, sg.C, 1, 1) for sg in segs]
    return xs, ws, [1 if sg.kind == "convT" else 0 for sg in segs]


def normal(B, M, segs, seed=0, bias=False, addend=False):
    OH, OW = _plan.seg_out(segs[0])
    return cr.job_inputs(B, M, segs, OH, OW, seed=seed, bias=bias, addend=addend)


UNIT = 2.0 ** -18     # every product of the integer builder is a multiple of it


def integer(B, M, segs, seed=0, bias=False, addend=False):
    """x and w are +-n 2^-9 with n odd in [257, 319]: nine significant bits, so hi = the top eight and mid = the
    last one, both nonzero (lo = 0), and a product is an integer below 319^2 times UNIT.  bias and addend are
    +-n 2^-9, n <= 198 (below one product).  With S = sum |w| |x| + |bias| + |addend| < 2^24 UNIT = 64 every
    partial sum in any order is an integer multiple of UNIT below 2^24: fp32 holds it exactly, whatever the
    order of the additions, and the kernel must equal the float64 reference bit for bit (asserted here)."""
    gen = torch.Generator().manual_seed(1000 + seed)
    OH, OW = _plan.seg_out(segs[0])

    def draw(shape, lo, hi, step):
        n = torch.randint(0, (hi - lo) // step + 1, shape, generator=gen) * step + lo
        sign = torch.randint(0, 2, shape, generator=gen) * 2 - 1
        return (n * sign).float() * 2.0 ** -9
    xs_, ws_, layouts = _shapes(B, M, segs)
    d = dict(xs=[draw(s, 257, 319, 2) for s in xs_], ws=[draw(s, 257, 319, 2) for s in ws_], layouts=layouts,
             gates=[None] * len(segs), bias=draw((M,), 1, 198, 1) if bias else None,
             addend=draw((B, M, OH, OW), 1, 198, 1) if addend else None)
    S = abs_sum_ref(segs, d)
    assert float(S.max()) < 2.0 ** 24 * UNIT, float(S.max())
    return d


def _full_significands(shape, gen):
    """float32 values with all 24 significand bits in use: random sign and mantissa, exponents 2^-6 .. 2^6, the
    first values those of conv_refs.split_inputs whose low bits are all set (0x3F7FFFFF among them)"""
    n = int(np.prod(shape))
    bits = torch.randint(0, 1 << 23, (n,), generator=gen) | 1
    bits |= torch.randint(121, 134, (n,), generator=gen) << 23
    bits |= torch.randint(0, 2, (n,), generator=gen) << 31
    a = bits.numpy().astype(np.uint32)
    ones = np.array([0x3F80FFFF, 0xBFFFFFFF, 0x40FFFFFF, 0x3F7FFFFF, 0xC2000001, 0x3F8000FF, 0x3F80FF01], dtype=np.uint32)
    a[:min(n, 7)] = ones[:n]
    return torch.from_numpy(a.view(np.float32).copy()).reshape(shape)


def onehot_w(B, M, segs, seed=0, bias=False, addend=False):
    """output channel m has one nonzero weight +-2^e (e in -3 .. 3) at segment m % nseg, one channel, one tap; x
    has full significands.  hi + mid + lo reconstructs x exactly and 2^e has a hi piece only, so every output
    element is one input element times a power of two (or zero where the tap falls outside): bitwise."""
    assert not bias and not addend
    gen = torch.Generator().manual_seed(2000 + seed)
    xs_, ws_, layouts = _shapes(B, M, segs)
    ws = [torch.zeros(s) for s in ws_]
    for m in range(M):
        si = m % len(segs)
        sg = segs[si]
        c = int(torch.randint(0, sg.C, (1,), generator=gen))
        v = float(2.0 ** int(torch.randint(-3, 4, (1,), generator=gen)) * (1 - 2 * int(torch.randint(0, 2, (1,), generator=gen))))
        if sg.kind == "convT":
            ws[si][c, m, (m // len(segs)) % 4, (m // (4 * len(segs)) + m) % 4] = v
        else:
            ws[si][m, c, 0, 0] = v
    return dict(xs=[_full_significands(s, gen) for s in xs_], ws=ws, layouts=layouts, gates=[None] * len(segs),
                bias=None, addend=None)


def onehot_x(B, M, segs, seed=0, bias=False, addend=False):
    """the mirror image: sample b has one nonzero input +-2^e, in segment b % nseg at one (channel, pixel), and
    the weights have full significands: every output element is one weight times a power of two, or zero"""
    assert not bias and not addend
    gen = torch.Generator().manual_seed(3000 + seed)
    xs_, ws_, layouts = _shapes(B, M, segs)
    xs = [torch.zeros(s) for s in xs_]
    for b in range(B):
        si = b % len(segs)
        sg = segs[si]
        c, y, x = (int(torch.randint(0, n, (1,), generator=gen)) for n in (sg.C, sg.IH, sg.IW))
        xs[si][b, c, y, x] = float(2.0 ** int(torch.randint(-3, 4, (1,), generator=gen)) * (1 - 2 * (b % 2)))
    return dict(xs=xs, ws=[_full_significands(s, gen) for s in ws_], layouts=layouts, gates=[None] * len(segs),
                bias=None, addend=None)


BUILDERS = {"normal": normal, "integer": integer, "onehot_w": onehot_w, "onehot_x": onehot_x}
