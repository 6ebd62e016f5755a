"""Seeded macroblock records and pictures for the loop-filter tests (test_spec_oracle_deblock.py on
the CPU, test_gpu_avc_deblock.py on the GPU), and the comparison helpers they share.

A case is built ONCE in the oracle's terms (tests/spec_oracle.py deblock_picture: one dict per
macroblock, separate Cb / Cr planes) and then packed into what native.avc_deblock_records takes
(per-field record arrays, the i16 vector pool, NV12 planes). No encoder and no decoder is involved,
so sparse patterns no stream of ours contains (one filtering MB in a disabled picture, non-zero
FilterOffsetA/B, 1-MB pictures) are reachable.

The numbers below that belong to the binding's record format (MbKind, MbRec::flags bits, the
granularity of the vector pool, dbk bits) are restated from csrc/vep/avc_recon.h's comments.
"""
from __future__ import annotations

import numpy as np

import spec_oracle as so

K_SKIP, K_INTER, K_I4, K_I16, K_PCM, K_I8 = 0, 1, 2, 3, 4, 5
F_T8, F_L1, F_MV8, F_MV16 = 1, 2, 8, 16
NOREF = 0xFF

_OFFS = [-12, -6, -4, -2, 0, 0, 0, 2, 4, 6, 12]


def _mv_step(rng, field, vertical):
    """0, or a step that puts the mv rule on its threshold: 3 / 4, and 1 / 2 vertically in fields."""
    steps = [0, 0, 0, 3, -3, 4, -4]
    if field and vertical:
        steps += [1, -1, 2, -2]
    return int(rng.choice(steps))


def _plane(rng, wmbs, hmbs, mbw, mbh, bd, peaks):
    """Per-MB base level + noise of spread 2 / 6 / 20 / 60 + steps of 0 / +-8 at 4x4 block edges
    (uniform noise would almost never pass the alpha / beta test); `peaks` MBs sit at 0 or at the
    top of the range."""
    sc = 1 << (bd - 8)
    mx = (1 << bd) - 1
    out = np.zeros((hmbs * mbh, wmbs * mbw), np.int32)
    prev = int(rng.integers(40, 200))
    for my in range(hmbs):
        for mxx in range(wmbs):
            a = my * wmbs + mxx
            # neighbouring MBs mostly close in level, so MB edges pass |p0 - q0| < alpha too
            base = prev + int(rng.choice([0, 0, 3, -3, 8, -8, 25, -25])) if rng.random() < 0.8 else int(rng.integers(0, 256))
            base = min(max(base, 0), 255)
            if a in peaks:
                base = 0 if peaks[a] == 0 else 255
            prev = base
            spread = int(rng.choice([2, 2, 6, 6, 20, 60]))
            blk = np.zeros((mbh, mbw), np.int32)
            for by in range(mbh // 4):
                for bx in range(mbw // 4):
                    blk[4 * by:4 * by + 4, 4 * bx:4 * bx + 4] = int(rng.choice([0, 0, 8, -8]))
            noise = rng.integers(-(spread // 2), spread // 2 + 1, (mbh, mbw))
            v = (base + blk + noise) * sc
            if a in peaks:  # exactly the range's end on part of the MB
                v[:, : mbw // 2] = 0 if peaks[a] == 0 else mx
            out[my * mbh:(my + 1) * mbh, mxx * mbw:(mxx + 1) * mbw] = np.clip(v, 0, mx)
    return out


def make_case(seed, wmbs, hmbs, ptype="B", bd=8, cf=1, field=0, pattern=None):
    """ptype 'I' (mostly intra MBs) or 'B' (mostly inter). pattern: None, 'all_off', 'checker' or
    ('only', mb address): overrides which MBs have the filter disabled."""
    rng = np.random.default_rng([seed, wmbs, hmbs, bd, field, 1 if ptype == "I" else 0])  # (not cf: 4:2:2 shares the records and luma)
    n = wmbs * hmbs
    bias = 6 * (bd - 8)
    # 1..4 slices of consecutive MBs, each with its idc and (even) filter offsets
    nsl = min(n, int(rng.integers(1, 5)))
    cuts = sorted(rng.choice(np.arange(1, n), nsl - 1, replace=False).tolist()) if nsl > 1 else []
    slice_of = np.searchsorted(np.array(cuts, np.int64), np.arange(n), side="right") if cuts else np.zeros(n, np.int64)
    sl_idc = [int(rng.choice([0, 0, 0, 1, 2, 2])) for _ in range(nsl)]
    if all(i == 1 for i in sl_idc):
        sl_idc[0] = 0
    sl_a = [int(rng.choice(_OFFS)) for _ in range(nsl)]
    sl_b = [int(rng.choice(_OFFS)) for _ in range(nsl)]

    mbs, kinds, flags, nzs, mv_off = [], [], [], [], []
    refs = np.full((n, 4), NOREF, np.int64)
    refs1 = np.full((n, 4), NOREF, np.int64)
    pool: list[int] = []
    p_intra = 0.75 if ptype == "I" else 0.15
    for a in range(n):
        mx, my = a % wmbs, a // wmbs
        s = int(slice_of[a])
        idc = sl_idc[s]
        if pattern == "all_off":
            idc = 1
        elif pattern == "checker":
            idc = 1 if (mx + my) & 1 else (0 if idc == 1 else idc)
        elif isinstance(pattern, tuple) and pattern[0] == "only":
            idc = 0 if a == pattern[1] else 1
        intra = rng.random() < p_intra
        if n == 2:  # a 2-MB picture reaches every bS only with one MB of each sort
            intra = a == seed % 2
        if intra:
            kind = int(rng.choice([K_I4, K_I16, K_I8, K_PCM]))
        else:
            kind = K_SKIP if rng.random() < 0.25 else K_INTER
        qpy = int(rng.integers(-bias, 52)) if rng.random() < 0.4 else int(rng.integers(18, 46))
        if kind == K_PCM:
            qpy = 0
        qpc = tuple(int(rng.integers(-bias, 40)) if rng.random() < 0.3 else int(rng.integers(16, 40)) for _ in range(2))
        t8 = kind == K_I8 or (kind == K_INTER and rng.random() < 0.4)
        coded = 0 if kind == K_SKIP else int(rng.choice([0, 0, int(rng.integers(0, 1 << 16)), int(rng.integers(0, 1 << 16)) & int(rng.integers(0, 1 << 16)) & int(rng.integers(0, 1 << 16))]))
        mb = {"intra": intra, "qp": qpy, "qpc": qpc, "idc": idc, "off_a": sl_a[s], "off_b": sl_b[s], "slice": s,
              "t8": bool(t8), "coded": coded, "motion": None}
        fl = F_T8 if t8 else 0
        off = 0
        if not intra:
            gran = F_MV16 if kind == K_SKIP else int(rng.choice([F_MV16, F_MV8, 0]))
            # the neighbour whose motion this MB mostly continues (so that bS 0 is dense)
            nb = None
            if mx > 0 and not mbs[a - 1]["intra"] and rng.random() < 0.7:
                nb = a - 1
            elif my > 0 and not mbs[a - wmbs]["intra"]:
                nb = a - wmbs
            if nb is not None and rng.random() < 0.6:
                l1 = bool(flags[nb] & F_L1)
                r0, r1 = refs[nb].copy(), refs1[nb].copy()
                b0 = list(mbs[nb]["_base"][0])
                b1 = list(mbs[nb]["_base"][1])
                if gran == F_MV16:
                    r0[:], r1[:] = r0[0], r1[0]
            else:
                l1 = rng.random() < 0.5
                pick = lambda: int(rng.choice([0, 1, 2, NOREF]))  # noqa: E731
                r0 = np.array([pick() for _ in range(4)], np.int64)
                r1 = np.array([pick() for _ in range(4)], np.int64) if l1 else np.full(4, NOREF, np.int64)
                if gran == F_MV16:
                    r0[:], r1[:] = r0[0], r1[0]
                for k in range(4):  # every partition predicts from something
                    if r0[k] == NOREF and (not l1 or r1[k] == NOREF):
                        r0[k] = int(rng.integers(0, 3))
                b0 = [int(rng.integers(-40, 41)), int(rng.integers(-40, 41))]
                b1 = list(b0) if rng.random() < 0.5 else [int(rng.integers(-40, 41)), int(rng.integers(-40, 41))]
            b0 = [b0[0] + _mv_step(rng, field, False), b0[1] + _mv_step(rng, field, True)]
            b1 = [b1[0] + _mv_step(rng, field, False), b1[1] + _mv_step(rng, field, True)]
            nvec = 1 if gran == F_MV16 else 4 if gran == F_MV8 else 16
            vecs = [[], []]
            for lst, b in ((0, b0), (1, b1)):
                for _ in range(nvec):
                    if rng.random() < 0.6:
                        vecs[lst].append((b[0], b[1]))
                    else:
                        vecs[lst].append((b[0] + _mv_step(rng, field, False), b[1] + _mv_step(rng, field, True)))
            if l1 and rng.random() < 0.3:  # both lists with the same vectors: the crossed pairing matters
                vecs[1] = list(vecs[0])
            motion = []
            for blk in range(16):
                by, bx = blk >> 2, blk & 3
                q8 = 2 * (by >> 1) + (bx >> 1)
                vi = 0 if gran == F_MV16 else q8 if gran == F_MV8 else blk
                m = []
                if r0[q8] != NOREF:
                    m.append((int(r0[q8]), vecs[0][vi]))
                if l1 and r1[q8] != NOREF:
                    m.append((int(r1[q8]), vecs[1][vi]))
                motion.append(m)
            mb["motion"] = motion
            mb["_base"] = (b0, b1)
            refs[a], refs1[a] = r0, r1
            fl |= gran | (F_L1 if l1 else 0)
            off = len(pool)
            if rng.random() < 0.2:  # a gap in the pool: offsets are not a running count
                pool += [0x7FFF] * 6
                off = len(pool)
            for lst in range(2 if l1 else 1):
                for v in vecs[lst]:
                    pool += [v[0], v[1]]
        # the record's nz is 8x8-consistent for 8x8-transform MBs; the oracle gets the raw mask
        nz = coded
        if t8:
            nz = 0
            for q8 in range(4):
                quad = [4 * (2 * (q8 >> 1) + j) + 2 * (q8 & 1) + i for j in (0, 1) for i in (0, 1)]
                if any((coded >> b) & 1 for b in quad):
                    for b in quad:
                        nz |= 1 << b
        mbs.append(mb)
        kinds.append(kind)
        flags.append(fl)
        nzs.append(nz)
        mv_off.append(off)

    peaks = {}
    if n >= 4:
        for a, v in zip(rng.choice(n, 2, replace=False).tolist(), (0, 1)):
            peaks[int(a)] = v
    y = _plane(rng, wmbs, hmbs, 16, 16, bd, peaks)
    ch = 16 if cf == 2 else 8
    cb = _plane(rng, wmbs, hmbs, 8, ch, bd, peaks)
    cr = _plane(rng, wmbs, hmbs, 8, ch, bd, {a: 1 - v for a, v in peaks.items()})
    dt = np.uint16 if bd > 8 else np.uint8
    uv = np.zeros((hmbs * ch, wmbs * 16), dt)
    uv[:, 0::2] = cb
    uv[:, 1::2] = cr
    recs = {
        "kind": np.array(kinds, np.int64),
        "qp": np.array([m["qp"] + bias for m in mbs], np.int64),
        "qpc": np.array([m["qpc"][0] + bias for m in mbs], np.int64),
        "qpc2": np.array([m["qpc"][1] + bias for m in mbs], np.int64),
        "dbk": np.array([{0: 0, 1: 1, 2: 2}[m["idc"]] for m in mbs], np.int64),
        "flags": np.array(flags, np.int64),
        "nz": np.array(nzs, np.int64),
        "alpha_off": np.array([m["off_a"] for m in mbs], np.int64),
        "beta_off": np.array([m["off_b"] for m in mbs], np.int64),
        "slice": np.array([m["slice"] for m in mbs], np.int64),
        "ref": refs,
        "ref1": refs1,
        "mv": np.array(mv_off, np.int64),
    }
    return {
        "name": f"{ptype}{wmbs}x{hmbs}-bd{bd}-cf{cf}-f{field}-{pattern}-s{seed}",
        "wmbs": wmbs, "hmbs": hmbs, "bd": bd, "cf": cf, "field": field, "pattern": pattern,
        "mbs": mbs, "y": y, "cb": cb, "cr": cr,
        "args": {"y": y.astype(dt), "uv": uv, "recs": recs, "mvs": np.array(pool, np.int16), "wmbs": wmbs,
                 "hmbs": hmbs, "bit_depth": bd, "chroma_format": cf, "field": field},
    }


def run_native(native, case, device=-1, variant=5):
    a = case["args"]
    return native.avc_deblock_records(a["y"], a["uv"], a["recs"], a["mvs"], a["wmbs"], a["hmbs"],
                                      bit_depth=a["bit_depth"], chroma_format=a["chroma_format"], field=a["field"],
                                      device=device, variant=variant)


def oracle(case):
    """(y, uv, stats, writer) of spec_oracle.deblock_picture on the case, computed once (4:2:0)."""
    if "_oracle" not in case:
        assert case["cf"] == 1, "the oracle covers 4:2:0 only"
        y, cb, cr = case["y"].copy(), case["cb"].copy(), case["cr"].copy()
        stats = so.new_deblock_stats()
        writer = [np.full(y.shape, -1, np.int32), np.full(cb.shape, -1, np.int32), np.full(cr.shape, -1, np.int32), []]
        so.deblock_picture(y, cb, cr, case["mbs"], case["wmbs"], case["hmbs"], field=case["field"] != 0,
                           bd=case["bd"], stats=stats, writer=writer)
        uv = np.zeros_like(case["args"]["uv"])
        uv[:, 0::2] = cb
        uv[:, 1::2] = cr
        case["_oracle"] = (y.astype(uv.dtype), uv, stats, writer)
    return case["_oracle"]


def check_honest(case):
    """The conditions that keep a case from passing vacuously, from the oracle alone."""
    y, uv, st, _ = oracle(case)
    a = case["args"]
    pat = case["pattern"]
    if pat == "all_off":
        assert np.array_equal(y, a["y"]) and np.array_equal(uv, a["uv"]), case["name"]
        return
    assert not np.array_equal(y, a["y"]), f"{case['name']}: the oracle leaves luma as it was"
    assert st["pass"] > 0 and st["fail"] > 0, f"{case['name']}: alpha/beta test {st}"
    assert st["chroma"][0] > 0 and st["chroma"][1] > 0, f"{case['name']}: chroma not filtered in both planes {st}"
    exempt = (isinstance(pat, tuple) and pat[0] == "only") or case["wmbs"] * case["hmbs"] == 1
    if not exempt:
        assert all(c > 0 for c in st["bs"]), f"{case['name']}: bS histogram {st['bs']}"
        assert st["bs4_strong"] > 0 and st["bs4_weak"] > 0, f"{case['name']}: bS 4 branches {st}"
        assert st["ap_lt"] > 0 and st["ap_ge"] > 0, f"{case['name']}: ap < beta outcomes {st}"


_PLANES = ("Y", "Cb", "Cr")


def explain(case, got_y, got_uv, want_y, want_uv, writer=None):
    """None when equal; else a message naming the first differing sample and, with the oracle's
    writer map, the MB / plane / edge / line whose filter last wrote it."""
    if np.array_equal(got_y, want_y) and np.array_equal(got_uv, want_uv):
        return None
    pairs = [(got_y, want_y), (got_uv[:, 0::2], want_uv[:, 0::2]), (got_uv[:, 1::2], want_uv[:, 1::2])]
    total = sum(int(np.count_nonzero(g != w)) for g, w in pairs)
    for c, (g, w) in enumerate(pairs):
        d = np.argwhere(g != w)
        if len(d) == 0:
            continue
        yy, xx = (int(v) for v in d[0])
        mbw = 16 if c == 0 else 8
        mbh = 16 if (c == 0 or case["cf"] == 2) else 8
        msg = (f"{case['name']}: {total} samples differ; first: plane {_PLANES[c]} x {xx} y {yy} "
               f"(MB column {xx // mbw} row {yy // mbh}, sample {xx % mbw},{yy % mbh} of it): "
               f"got {int(g[yy, xx])}, want {int(w[yy, xx])}, input {int((case['y'], case['cb'], case['cr'])[c][yy, xx])}")
        if writer is not None:
            i = int(writer[c][yy, xx])
            if i < 0:
                msg += "; the reference filters no edge over this sample"
            else:
                addr, pc, d_, e, k = writer[3][i]
                msg += (f"; last written in the reference by MB {addr} (column {addr % case['wmbs']} row "
                        f"{addr // case['wmbs']}) plane {_PLANES[pc]} {'horizontal' if d_ else 'vertical'} edge {e} line {k}")
        return msg
    return None



# ------------------------------------------------------------------ directed two-MB pictures
def side(ref0=NOREF, ref1=NOREF, mv0=(0, 0), mv1=(0, 0), coded=0, t8=False, intra=False):
    """One MB with uniform motion, at record level: DPB slots of list 0 / list 1 (NOREF: unused)
    and their vectors."""
    return {"ref0": ref0, "ref1": ref1, "mv0": mv0, "mv1": mv1, "coded": coded, "t8": t8, "intra": intra}


def side_block(s, blk=0):
    """The side as spec_oracle.boundary_strength sees one of its 4x4 blocks."""
    m = []
    if s["ref0"] != NOREF:
        m.append((s["ref0"], s["mv0"]))
    if s["ref1"] != NOREF:
        m.append((s["ref1"], s["mv1"]))
    mb = {"intra": s["intra"], "t8": s["t8"], "coded": s["coded"], "motion": [m] * 16}
    return so._block(mb, blk)


def directed_case(p, q, vertical=True, field=0, bd=8):
    """A picture of two MBs, p then q (side by side, or q below p), flat at two levels 32 apart at
    QP 40 (alpha 80, beta 13, tC0 4 / 5 / 7), so that the bS of the MB edge between them decides
    p0: bS 0 leaves 100, bS 1 / 2 / 3 clip the change of 12 at tC0 + 2 = 6 / 7 / 9, bS 4 takes the
    weak filter (32 >= (alpha >> 2) + 2) and gives 108."""
    wmbs, hmbs = (2, 1) if vertical else (1, 2)
    sc = 1 << (bd - 8)
    bias = 6 * (bd - 8)
    mbs, pool, mv_off, flags, nzs = [], [], [], [], []
    for s in (p, q):
        blkinfo = []
        for blk in range(16):
            blkinfo.append(side_block(s, blk)["motion"])
        mbs.append({"intra": s["intra"], "qp": 40, "qpc": (36, 33), "idc": 0, "off_a": 0, "off_b": 0, "slice": 0,
                    "t8": s["t8"], "coded": s["coded"], "motion": None if s["intra"] else blkinfo})
        l1 = s["ref1"] != NOREF
        flags.append((F_T8 if s["t8"] else 0) | (0 if s["intra"] else F_MV16 | (F_L1 if l1 else 0)))
        mv_off.append(len(pool))
        if not s["intra"]:
            pool += list(s["mv0"]) + (list(s["mv1"]) if l1 else [])
        nz = s["coded"]
        if s["t8"]:
            nz = 0
            for q8 in range(4):
                quad = [4 * (2 * (q8 >> 1) + j) + 2 * (q8 & 1) + i for j in (0, 1) for i in (0, 1)]
                if any((s["coded"] >> b) & 1 for b in quad):
                    nz |= sum(1 << b for b in quad)
        nzs.append(nz)

    def two_level(h, w):
        a = np.full((h, w), 100 * sc, np.int32)
        if vertical:
            a[:, w // 2:] = 132 * sc
        else:
            a[h // 2:, :] = 132 * sc
        return a

    y, cb, cr = two_level(hmbs * 16, wmbs * 16), two_level(hmbs * 8, wmbs * 8), two_level(hmbs * 8, wmbs * 8)
    dt = np.uint16 if bd > 8 else np.uint8
    uv = np.zeros((hmbs * 8, wmbs * 16), dt)
    uv[:, 0::2] = cb
    uv[:, 1::2] = cr
    sides = (p, q)
    recs = {
        "kind": np.array([K_I16 if s["intra"] else K_INTER for s in sides], np.int64),
        "qp": np.array([40 + bias] * 2, np.int64), "qpc": np.array([36 + bias] * 2, np.int64),
        "qpc2": np.array([33 + bias] * 2, np.int64), "dbk": np.zeros(2, np.int64), "flags": np.array(flags, np.int64),
        "nz": np.array(nzs, np.int64), "alpha_off": np.zeros(2, np.int64), "beta_off": np.zeros(2, np.int64),
        "slice": np.zeros(2, np.int64),
        "ref": np.array([[NOREF if s["intra"] else s["ref0"]] * 4 for s in sides], np.int64),
        "ref1": np.array([[NOREF if s["intra"] else s["ref1"]] * 4 for s in sides], np.int64),
        "mv": np.array(mv_off, np.int64),
    }
    return {
        "name": f"directed-{'v' if vertical else 'h'}-f{field}", "wmbs": wmbs, "hmbs": hmbs, "bd": bd, "cf": 1,
        "field": field, "pattern": None, "mbs": mbs, "y": y, "cb": cb, "cr": cr,
        "args": {"y": y.astype(dt), "uv": uv, "recs": recs, "mvs": np.array(pool or [0, 0], np.int16), "wmbs": wmbs,
                 "hmbs": hmbs, "bit_depth": bd, "chroma_format": 1, "field": field},
    }


A, B_, FAR = (8, -4), (-20, 12), (30, 30)
# (name, p, q, bS of a vertical MB edge in a frame, ... horizontal MB edge in a field picture)
BS_TABLE = [
    ("intra p", side(intra=True), side(0), 4, 3),
    ("intra q", side(1), side(intra=True), 4, 3),
    ("coefficients in p's block", side(0, coded=1 << 3 | 1 << 12), side(0), 2, 2),  # blocks 3 / 12 border the edge
    ("coefficients in q's block", side(0), side(0, coded=0xFFFF), 2, 2),
    ("8x8 transform: coefficients elsewhere in p's 8x8", side(0, coded=1 << 6, t8=True), side(0), 2, 0),
    ("4x4 transform: coefficients elsewhere in p's 8x8", side(0, coded=1 << 6), side(0), 0, 0),
    ("different reference pictures", side(0, mv0=A), side(1, mv0=A), 1, 1),
    ("different number of vectors", side(0, mv0=A), side(0, 1, mv0=A, mv1=A), 1, 1),
    ("same picture, same vector", side(0, mv0=A), side(0, mv0=A), 0, 0),
    ("mv x differs by 3", side(0, mv0=A), side(0, mv0=(A[0] + 3, A[1])), 0, 0),
    ("mv x differs by 4", side(0, mv0=A), side(0, mv0=(A[0] - 4, A[1])), 1, 1),
    ("mv y differs by 1", side(0, mv0=A), side(0, mv0=(A[0], A[1] + 1)), 0, 0),
    ("mv y differs by 2", side(0, mv0=A), side(0, mv0=(A[0], A[1] - 2)), 0, 1),   # field: 2 quarter field samples
    ("mv y differs by 3", side(0, mv0=A), side(0, mv0=(A[0], A[1] + 3)), 0, 1),
    ("mv y differs by 4", side(0, mv0=A), side(0, mv0=(A[0], A[1] + 4)), 1, 1),
    ("one picture through list 0 and list 1", side(2, mv0=A), side(NOREF, 2, mv1=A), 0, 0),
    ("... with distant vectors", side(2, mv0=A), side(NOREF, 2, mv1=FAR), 1, 1),
    ("... and another picture", side(2, mv0=A), side(NOREF, 1, mv1=A), 1, 1),
    ("two pictures, same way round", side(0, 1, A, B_), side(0, 1, A, B_), 0, 0),
    ("two pictures, crossed", side(0, 1, A, B_), side(1, 0, B_, A), 0, 0),
    ("two pictures, crossed, vectors not", side(0, 1, A, B_), side(1, 0, A, B_), 1, 1),
    ("two pictures, one vector 4 away", side(0, 1, A, B_), side(0, 1, A, (B_[0] + 4, B_[1])), 1, 1),
    ("two pictures against a pair with one other", side(0, 1, A, B_), side(0, 2, A, B_), 1, 1),
    ("one picture twice against two pictures", side(0, 0, A, B_), side(0, 1, A, B_), 1, 1),
    ("one picture twice, same way round", side(0, 0, A, B_), side(0, 0, A, B_), 0, 0),
    ("one picture twice, crossed", side(0, 0, A, B_), side(0, 0, B_, A), 0, 0),
    ("one picture twice, neither pairing", side(0, 0, A, B_), side(0, 0, A, FAR), 1, 1),
    ("one picture twice, straight pairing 3 / crossed far", side(0, 0, A, B_), side(0, 0, (A[0] + 3, A[1]), B_), 0, 0),
]


# ------------------------------------------------------------------ the cases both test files run
# Shapes in MBs, from the structure of avc_deblock_kernel: a wave filters two MB rows, a workgroup
# 8 rows, the LDS exchange ring is 8 columns deep.
SHAPES = [(1, 1), (2, 1), (1, 2), (3, 3),   # lone MB / row / column; odd row count (a lone last row)
          (9, 2), (17, 3),                  # the ring wraps once / twice (back-pressure path)
          (1, 9), (2, 17),                  # one / two workgroup hand-offs, width at or below the lag
          (10, 16),                         # two full workgroups
          (17, 9)]                          # ring wrap + hand-off + odd row in the second group
BIG = (17, 9)
HBD_SHAPES = [(1, 1), (2, 1), (1, 2), (3, 3), (9, 2), (17, 3), (33, 17)]  # 33x17: a diagonal of 17 MBs
MANY_HEIGHTS = [1, 2, 3, 8, 9, 16, 17, 9, 1]
MANY_WIDTHS = [3, 17, 1, 9, 2, 5, 4, 10, 33]

# Seeds chosen (tests/deblock_cases.py --seeds prints them) so that every case meets check_honest
# from the oracle alone; anything not listed uses seed 1.
SEEDS: dict = {
    ('B', 1, 1, 10, 1, 0, None): 6,
    ('B', 1, 1, 8, 1, 0, None): 3,
    ('B', 1, 2, 10, 1, 0, None): 8,
    ('B', 1, 2, 8, 1, 0, None): 34,
    ('B', 1, 9, 8, 1, 0, None): 3,
    ('B', 17, 9, 10, 1, 0, ('only', 0)): 6,
    ('B', 17, 9, 10, 1, 0, ('only', 127)): 4,
    ('B', 17, 9, 10, 1, 0, ('only', 136)): 2,
    ('B', 17, 9, 8, 1, 0, ('only', 0)): 17,
    ('B', 17, 9, 8, 1, 0, ('only', 136)): 8,
    ('B', 2, 1, 10, 1, 0, None): 69,
    ('B', 2, 1, 8, 1, 0, None): 35,
    ('B', 3, 3, 8, 1, 0, None): 2,
    ('B', 9, 2, 10, 1, 0, None): 2,
    ('B', 9, 2, 8, 1, 0, None): 2,
    ('I', 1, 1, 10, 1, 0, None): 2,
    ('I', 1, 1, 8, 1, 0, None): 2,
    ('I', 1, 2, 10, 1, 0, None): 55,
    ('I', 1, 2, 8, 1, 0, None): 152,
    ('I', 1, 3, 10, 1, 0, None): 91,
    ('I', 1, 3, 8, 1, 0, None): 19,
    ('I', 1, 9, 8, 1, 0, None): 3,
    ('I', 17, 9, 10, 1, 0, ('only', 144)): 13,
    ('I', 17, 9, 10, 1, 0, ('only', 152)): 2,
    ('I', 17, 9, 8, 1, 0, ('only', 144)): 3,
    ('I', 17, 9, 8, 1, 0, ('only', 152)): 3,
    ('I', 2, 1, 10, 1, 0, None): 221,
    ('I', 2, 1, 8, 1, 0, None): 87,
    ('I', 2, 9, 10, 1, 0, None): 2,
    ('I', 3, 1, 10, 1, 0, None): 10,
    ('I', 3, 1, 8, 1, 0, None): 17,
    ('I', 3, 3, 10, 1, 0, None): 3,
    ('I', 3, 3, 8, 1, 0, None): 5,
    ('I', 9, 2, 10, 1, 0, None): 2,
    ('I', 9, 2, 8, 1, 0, None): 3,
}

_cache: dict = {}


def get_case(ptype, w, h, bd=8, cf=1, field=0, pattern=None):
    key = (ptype, w, h, bd, cf, field, pattern)
    if key not in _cache:
        # (4:2:2 cases share the 4:2:0 case's seed: the oracle does not judge them)
        seed = SEEDS.get((ptype, w, h, bd, 1, field, pattern), 1)
        _cache[key] = make_case(seed, w, h, ptype, bd, cf, field, pattern)
    return _cache[key]


def only_addresses(w=BIG[0], h=BIG[1]):
    """'Only one MB filters': the four corners, and rows 7 / 8 either side of the hand-off."""
    return [0, w - 1, (h - 1) * w, h * w - 1, 7 * w + w // 2, 8 * w + w // 2]


def cases_420(bd=8):
    """Every 4:2:0 case (the oracle judges all of them) as get_case argument tuples."""
    out = []
    shapes = SHAPES if bd == 8 else HBD_SHAPES
    for w, h in shapes:
        for pt in ("I", "B"):
            out.append((pt, w, h, bd, 1, 0, None))
    w, h = BIG
    out += [("B", w, h, bd, 1, 0, "all_off"), ("B", w, h, bd, 1, 0, "checker"), ("I", w, h, bd, 1, 0, "checker")]
    out += [("I" if i & 1 else "B", w, h, bd, 1, 0, ("only", a)) for i, a in enumerate(only_addresses())]
    out += [("B", w, h, bd, 1, 1, None), ("I", w, h, bd, 1, 2, None)]
    return out


def many_cases(bd=8, cf=1):
    return [get_case("B" if i & 1 else "I", MANY_WIDTHS[i], hh, bd, cf) for i, hh in enumerate(MANY_HEIGHTS)]


def case_id(t):
    pt, w, h, bd, cf, field, pat = t
    s = f"{pt}{w}x{h}"
    if bd != 8:
        s += f"-{bd}bit"
    if cf != 1:
        s += "-422"
    if field:
        s += f"-field{field}"
    if pat:
        s += "-" + (pat if isinstance(pat, str) else f"only{pat[1]}")
    return s


if __name__ == "__main__":  # python tests/deblock_cases.py --seeds: search the SEEDS table
    found = {}
    todo = set(cases_420(8) + cases_420(10))
    for i, hh in enumerate(MANY_HEIGHTS):
        for bd in (8, 10):
            todo.add(("B" if i & 1 else "I", MANY_WIDTHS[i], hh, bd, 1, 0, None))
    for t in sorted(todo, key=repr):
        for seed in range(1, 400):
            c = make_case(seed, t[1], t[2], t[0], t[3], 1, t[5], t[6])
            try:
                check_honest(c)
            except AssertionError:
                continue
            if seed != 1:
                found[t] = seed
            break
        else:
            raise SystemExit(f"no seed for {t}")
    print("SEEDS: dict = {")
    for k, v in sorted(found.items(), key=repr):
        print(f"    {k!r}: {v},")
    print("}")
