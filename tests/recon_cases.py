"""Hand-built, seeded macroblock-record pictures for the reconstruction-records tests
(test_spec_oracle_recon.py on the CPU, test_gpu_avc_recon.py on the GPU).

A case is built once in the oracle's terms (recon_oracle.py: dicts that name reference pictures,
vectors, weights, modes and coefficients) and translated here into the arguments of
native.avc_recon_records: this file is the only place that knows both vocabularies. Shapes follow
the kernels' structure (64-MB chunks of a row, LDS lines up to 240 MBs, eight rows per workgroup);
the patterns are ones no stream of the project's encoders contains.
"""
from __future__ import annotations

import time

import numpy as np

import recon_oracle as ro

NOREF = 0xFF
K_SKIP, K_INTER, K_I4, K_I16, K_PCM, K_I8 = 0, 1, 2, 3, 4, 5
F_T8, F_L1, F_WP, F_MV8, F_MV16 = 1, 2, 4, 8, 16

FORMATS = [(8, 1), (10, 1), (8, 2), (10, 2)]  # (bit depth, chroma_format_idc); the first is the hot path
HBD_SHAPES = [(1, 1), (2, 1), (1, 2), (3, 3), (9, 2), (17, 3), (33, 17)]
MANY_HEIGHTS = [1, 2, 3, 8, 9, 16, 17, 9, 1]
MANY_WIDTHS = [3, 17, 1, 9, 2, 5, 4, 10, 33]
WIDE = [1, 2, 63, 64, 65, 66, 129, 240, 241]
TALL = [1, 2, 7, 8, 9, 16, 17]


def _hc(cf):
    return 8 if cf == 1 else 16


def _planes(rng, wmbs, hmbs, bd, cf, peaks=True):
    """Noise with flat patches at 0 and at the maximum (both clips of a weighted sample happen)."""
    mx = (1 << bd) - 1
    out = []
    for h, w in ((hmbs * 16, wmbs * 16), (hmbs * _hc(cf), wmbs * 8), (hmbs * _hc(cf), wmbs * 8)):
        p = rng.integers(0, mx + 1, size=(h, w), dtype=np.int64)
        if peaks:
            for v in (0, mx, 0, mx):
                y0, x0 = int(rng.integers(0, h)), int(rng.integers(0, w))
                p[y0:y0 + 6, x0:x0 + 6] = v
        out.append(p)
    return out


# ------------------------------------------------------------------ coefficients
def _fits(fn, d, bd):
    try:
        fn(d, bd)
        return True
    except AssertionError:
        return False


def _block(rng, n, bd, how):
    """n x n scaled coefficients of one transform block that pass the conformance range rule (drawn
    large, halved until the oracle's assertion holds)."""
    # (the records hold int16 coefficients: above 8 bits the standard's limit of 2 ** (7 + bd) is
    # beyond what a record can carry, and the binding refuses such a value)
    lim = min(1 << (7 + bd), 1 << 15)
    d = np.zeros((n, n), dtype=np.int64)
    if how == "limit":  # the extreme values the standard allows for an input coefficient
        d[0, 0] = lim - 1 if rng.integers(0, 2) else -lim
    elif how == "sparse":
        for _ in range(int(rng.integers(1, 4))):
            d[int(rng.integers(0, n)), int(rng.integers(0, n))] = int(rng.integers(-lim // 8, lim // 8))
    else:  # full
        d = rng.integers(-lim // 4, lim // 4, size=(n, n), dtype=np.int64)
    fn = ro.residual_4x4 if n == 4 else ro.residual_8x8
    while not _fits(fn, d.tolist(), bd):
        d = np.sign(d) * (np.abs(d) // 2)  # (towards zero)
    return d.tolist()


def _residual(rng, mb, bd, cf, how):
    """how: none | sparse | full | limit | chroma (chroma only) | mixed."""
    mb["luma"], mb["chroma"] = {}, {}
    if how == "none":
        return
    t8 = mb.get("t8", False)
    nl, n = (4, 8) if t8 else (16, 4)
    nbc = 4 if cf == 1 else 8
    for blk in range(nl):
        if how == "chroma":
            break
        h = how if how != "mixed" else ("none", "sparse", "full", "limit")[int(rng.integers(0, 4))]
        if h == "none" or (how == "sparse" and rng.integers(0, 3)):
            continue
        mb["luma"][blk] = _block(rng, n, bd, h)
    for c in range(2):
        for blk in range(nbc):
            h = "full" if how == "chroma" else how
            h = h if h != "mixed" else ("none", "sparse", "full", "limit")[int(rng.integers(0, 4))]
            if h == "none" or (how == "sparse" and rng.integers(0, 3)):
                continue
            mb["chroma"][(c, blk)] = _block(rng, 4, bd, h)


# ------------------------------------------------------------------ macroblocks in the oracle's terms
def pcm_mb(rng, bd, cf, slice_=0):
    mx = (1 << bd) - 1
    return {"type": "pcm", "slice": slice_, "y": rng.integers(0, mx + 1, (16, 16)), "cb": rng.integers(0, mx + 1, (_hc(cf), 8)),
            "cr": rng.integers(0, mx + 1, (_hc(cf), 8))}


def skip_mb(ref, slice_=0):
    """Zero-vector copy of one reference (a P_Skip with no neighbours)."""
    part = {"l0": (ref, [(0, 0)] * 4), "l1": None, "w": None}
    return {"type": "inter", "slice": slice_, "gran": 16, "skip": True, "t8": False, "luma": {}, "chroma": {},
            "parts": [dict(part) for _ in range(4)]}


def inter_mb(vec, gran, lists, refs, weights=None, slice_=0, t8=False):
    """vec(list, b8, sb) -> (mvx, mvy); gran 16 / 8 / 4: the vectors must then be uniform per MB / per
    8x8 (the caller's vec sees b8 = sb = 0, or sb = 0). lists[b8] in 'P', 'B', '0', '1' ('0': list 0
    only, '1': list 1 only, within a B macroblock); refs[list][b8]: reference names."""
    parts = []
    for b8 in range(4):
        p = {"w": None if weights is None else weights[b8]}
        for li, key in enumerate(("l0", "l1")):
            used = lists[b8] in ("P", "0", "B") if li == 0 else lists[b8] in ("1", "B")
            p[key] = None if not used else (refs[li][b8], [vec(li, 0 if gran == 16 else b8, 0 if gran > 4 else sb) for sb in range(4)])
        parts.append(p)
    return {"type": "inter", "slice": slice_, "gran": gran, "t8": t8, "parts": parts, "luma": {}, "chroma": {}}


def _weight(rng, how, bi):
    """Three per-component weight dicts; how: 'explicit' | 'implicit' | ('fixed', lwd, w0, w1, o0, o1)."""
    out = []
    for _ in range(3):
        if how == "implicit":  # (64 - w, w), logWD 5, no offsets; w in -64 .. 128
            w = int(rng.choice([-64, -1, 0, 1, 32, 63, 64, 127, 128]))
            out.append({"lwd": 5, "w0": 64 - w, "w1": w, "o0": 0, "o1": 0})
            continue
        if isinstance(how, tuple):
            _, lwd, w0, w1, o0, o1 = how
        else:
            lwd = int(rng.choice([0, 1, 5, 7]))
            pool = [-128, -1, 0, 1, 127] + ([128] if lwd == 7 else [])  # (128 = the default 1 << logWD at 7)
            w0, w1 = int(rng.choice(pool)), int(rng.choice(pool))
            o0, o1 = int(rng.choice([-128, -1, 0, 127])), int(rng.choice([-128, 0, 1, 127]))
        if bi:  # (7.4.3.2: -128 <= w0 + w1 <= (logWD == 7 ? 127 : 128))
            while not -128 <= w0 + w1 <= (127 if lwd == 7 else 128):
                w0, w1 = (int(w0 / 2), 0) if w1 == 0 else (w0, int(w1 / 2))  # (towards zero)
        out.append({"lwd": lwd, "w0": w0, "w1": w1, "o0": o0, "o1": o1})
    return out


def intra_mb(rng, pic, addr, kind, bd, cf, how="mixed"):
    """A random intra MB whose modes are drawn among those the availability allows (availability
    by the oracle's 6.4.11 / 6.4.12 functions). pic['mbs'] must already hold every MB's type and
    slice."""
    mb = pic["mbs"][addr]
    mb["type"] = kind
    mb["t8"] = kind == "i8"
    nb = ro.mb_neighbours(pic, addr)
    A, B, D = (ro.intra_usable(pic, nb[k]) for k in "ABD")
    mb["cmode"] = int(rng.choice(ro.allowed_modes(ro._NEEDSC, B, A, D)))
    if kind == "i16":
        mb["mode"] = int(rng.choice(ro.allowed_modes(ro._NEEDS16, B, A, D)))
    else:
        n = 4 if kind == "i4" else 8
        mb["modes"] = [int(rng.choice(ro.allowed_modes(ro._NEEDS, *ro.block_availability(pic, addr, (r % (16 // n)) * n,
                                                                                        (r // (16 // n)) * n))))
                       for r in range((16 // n) ** 2)]
    _residual(rng, mb, bd, cf, how)
    return mb


# ------------------------------------------------------------------ oracle terms -> binding arguments
def to_args(pic, init, nslots, target):
    """The arguments of native.avc_recon_records for `pic`; reference names are DPB slots."""
    wmbs, hmbs, bd, cf = pic["wmbs"], pic["hmbs"], pic["bd"], pic["cf"]
    n, hc, nbc = wmbs * hmbs, _hc(cf), 4 if cf == 1 else 8
    dt = np.uint16 if bd > 8 else np.uint8
    y = np.zeros((nslots, hmbs * 16, wmbs * 16), dtype=dt)
    uv = np.zeros((nslots, hmbs * hc, wmbs * 16), dtype=dt)
    for s in range(nslots):
        src = init if s == target else (pic["refs"][s]["y"], pic["refs"][s]["cb"], pic["refs"][s]["cr"])
        y[s] = src[0]
        uv[s][:, 0::2] = src[1]
        uv[s][:, 1::2] = src[2]
    recs = {k: np.zeros(n, dtype=np.int64) for k in ("kind", "flags", "slice", "mv", "i16_mode", "chroma_mode", "luma_coded",
                                                      "chroma_coded", "wp")}
    recs["ref"] = np.full((n, 4), NOREF, dtype=np.int64)
    recs["ref1"] = np.full((n, 4), NOREF, dtype=np.int64)
    recs["i4"] = np.zeros((n, 16), dtype=np.int64)
    coefs = np.zeros((n, 512), dtype=np.int64)
    mvs, wps = [], {"w0": [], "w1": [], "o": [], "lwd": []}
    sc = 1 << (bd - 8)
    for a, mb in enumerate(pic["mbs"]):
        recs["slice"][a] = mb["slice"]
        t = mb["type"]
        if t == "pcm":
            recs["kind"][a] = K_PCM
            coefs[a, :256 + 16 * hc] = np.concatenate([np.asarray(mb[k]).ravel() for k in ("y", "cb", "cr")])
            continue
        if t == "inter":
            flags = {16: F_MV16, 8: F_MV8, 4: 0}[mb["gran"]]
            l1 = any(p["l1"] is not None for p in mb["parts"])
            flags |= F_L1 if l1 else 0
            recs["mv"][a] = len(mvs)
            for key in ("l0", "l1")[:2 if l1 else 1]:
                # a list a partition does not use still has entries in the pool: far-away values a
                # kernel must not read
                vecs = [[(1999, -1777)] * 4 if p[key] is None else p[key][1] for p in mb["parts"]]
                if mb["gran"] == 16:
                    use = next((v[0] for v, p in zip(vecs, mb["parts"]) if p[key] is not None), vecs[0][0])
                    mvs += list(use)
                elif mb["gran"] == 8:
                    for v in vecs:
                        mvs += list(v[0])
                else:  # raster 4x4 blocks
                    for r in range(16):
                        b8, sb = (r // 8) * 2 + (r % 4) // 2, ((r // 4) % 2) * 2 + r % 2
                        mvs += list(vecs[b8][sb])
            for b8, p in enumerate(mb["parts"]):
                recs["ref"][a, b8] = NOREF if p["l0"] is None else p["l0"][0]
                recs["ref1"][a, b8] = NOREF if p["l1"] is None else p["l1"][0]
            if mb["parts"][0]["w"] is not None:
                flags |= F_WP
                recs["wp"][a] = len(wps["lwd"]) // 3
                for p in mb["parts"]:
                    bi = p["l0"] is not None and p["l1"] is not None
                    for e in p["w"]:
                        wps["w0"].append(e["w0"])
                        wps["w1"].append(e["w1"])
                        wps["lwd"].append(e["lwd"])
                        o0, o1 = e["o0"] * sc, e["o1"] * sc
                        wps["o"].append((o0 + o1 + 1) >> 1 if bi else (o0 if p["l0"] is not None else o1))
            recs["kind"][a] = K_SKIP if mb.get("skip") else K_INTER
        else:
            recs["kind"][a] = {"i4": K_I4, "i8": K_I8, "i16": K_I16}[t]
            flags = 0
            recs["chroma_mode"][a] = mb["cmode"]
            if t == "i16":
                recs["i16_mode"][a] = mb["mode"]
            else:
                recs["i4"][a, :len(mb["modes"])] = mb["modes"]
        if mb.get("t8"):
            flags |= F_T8
        recs["flags"][a] = flags
        for blk, d in mb.get("luma", {}).items():
            if mb.get("t8"):
                coefs[a, 64 * blk:64 * blk + 64] = np.asarray(d).ravel()
                recs["luma_coded"][a] |= 0x33 << ((blk & 1) * 2 + (blk >> 1) * 8)
            else:
                coefs[a, 16 * blk:16 * blk + 16] = np.asarray(d).ravel()
                recs["luma_coded"][a] |= 1 << blk
        for (c, blk), d in mb.get("chroma", {}).items():
            k = c * nbc + blk
            coefs[a, 256 + 16 * k:256 + 16 * k + 16] = np.asarray(d).ravel()
            recs["chroma_coded"][a] |= 1 << k
    return {"y": y, "uv": uv, "recs": recs, "mvs": np.asarray(mvs, dtype=np.int16), "wps": {k: np.asarray(v, dtype=np.int64) for k, v in wps.items()},
            "coefs": coefs, "wmbs": wmbs, "hmbs": hmbs, "slots": nslots, "target": target, "bit_depth": bd,
            "chroma_format": cf, "field": pic["field"], "constrained_intra": int(pic["constrained"])}


# ------------------------------------------------------------------ pictures
def _new_pic(rng, wmbs, hmbs, bd, cf, nrefs=2, field=0, constrained=False, target=None):
    """An empty picture with nrefs reference pictures named by their DPB slots; the target takes
    the slot `target` (default: the last). Field pictures: the slot's parity is the field's."""
    nslots = nrefs + 1
    target = nslots - 1 if target is None else target
    refs = {}
    for s in range(nslots):
        if s != target:
            yy, cb, cr = _planes(rng, wmbs, hmbs, bd, cf)
            refs[s] = {"y": yy, "cb": cb, "cr": cr, "bottom": bool(s & 1)}
    pic = {"wmbs": wmbs, "hmbs": hmbs, "bd": bd, "cf": cf, "field": field, "constrained": constrained, "refs": refs,
           "mbs": [None] * (wmbs * hmbs)}
    return pic, nslots, target


def _finish(name, pic, nslots, target, rng, expect=None):
    init = _planes(rng, pic["wmbs"], pic["hmbs"], pic["bd"], pic["cf"], peaks=False)
    return {"name": name, "pic": pic, "init": init, "args": to_args(pic, init, nslots, target), "expect": expect or {},
            "target": target}


def _seed(name, bd, cf):
    return abs(hash_name(name)) + 1000 * bd + cf


def hash_name(name):  # (str hashes are salted per process)
    v = 0
    for ch in name:
        v = (v * 131 + ord(ch)) % (1 << 31)
    return v


def _slices_by_rows(wmbs, hmbs, nslices, offset=0):
    """Slice boundaries at MB addresses that are NOT row starts (offset), nslices slices."""
    n = wmbs * hmbs
    cuts = [min(n, (k * n) // nslices + (offset if k else 0)) for k in range(nslices + 1)]
    out = []
    for a in range(n):
        out.append(max(k for k in range(nslices) if cuts[k] <= a))
    return out


def inter_case(name, bd, cf):
    """name: inter_<what>; small pictures of inter MBs."""
    rng = np.random.default_rng(_seed(name, bd, cf))
    what = name.split("_", 1)[1]
    expect = {}
    if what == "frac":  # 2 x 2 MBs, a vector per 4x4 block: all 64 (x, y) eighth positions, so all 16 quarter ones
        pic, ns, tg = _new_pic(rng, 2, 2, bd, cf)
        for a in range(4):
            def vec(li, b8, sb, a=a):
                k = a * 16 + b8 * 4 + sb
                return (8 * int(rng.integers(-2, 3)) + (k & 7) if li == 0 else int(rng.integers(-40, 40)),
                        8 * int(rng.integers(-2, 3)) + (k >> 3) if li == 0 else int(rng.integers(-40, 40)))
            lists = ["P"] * 4 if a < 2 else ["B"] * 4
            pic["mbs"][a] = inter_mb(vec, 4, lists, [[0] * 4, [1] * 4])
            _residual(rng, pic["mbs"][a], bd, cf, ("none", "sparse", "full", "chroma")[a])
        expect = {"frac": True}
    elif what == "far":  # 3 x 3: the block lies a picture or more outside, on every side and corner
        pic, ns, tg = _new_pic(rng, 3, 3, bd, cf)
        dirs = [(-1, 0), (1, 0), (0, -1), (0, 1), (-1, -1), (1, -1), (-1, 1), (1, 1), (0, 0)]
        for a, (dx, dy) in enumerate(dirs):
            far = (dx * (4 * 150 + int(rng.integers(0, 4))), dy * (4 * 110 + int(rng.integers(0, 4))))
            lim = (dx * 4 * 2040, dy * 4 * 500)  # near the level limits of the vector range
            pic["mbs"][a] = inter_mb(lambda li, b8, sb, far=far, lim=lim: far if li == 0 else lim, 16, ["B"] * 4, [[0] * 4, [1] * 4])
            _residual(rng, pic["mbs"][a], bd, cf, "sparse")
        expect = {"clamp": ["left", "right", "top", "bottom"]}
    elif what == "edge":  # 2 x 2: vectors one sample inside / outside each picture edge
        pic, ns, tg = _new_pic(rng, 2, 2, bd, cf)
        for a in range(4):
            sx, sy = (-1 if a % 2 == 0 else 1), (-1 if a // 2 == 0 else 1)

            def vec(li, b8, sb, sx=sx, sy=sy):
                d = 1 if li == 0 else 0  # list 0 one sample outside, list 1 exactly at the edge
                return (4 * sx * d + (b8 == 3 and li == 0), 4 * sy * d + 2 * (b8 == 1))
            pic["mbs"][a] = inter_mb(vec, 8, ["B", "0", "1", "B"], [[0, 1, 0, 1], [1, 1, 0, 0]])
            _residual(rng, pic["mbs"][a], bd, cf, "none")
        expect = {"clamp": ["left", "right", "top", "bottom"]}
    elif what.startswith("parts"):  # every record shape on 1x1, 2x1, 1x2, 3x3
        w, h = {"parts11": (1, 1), "parts21": (2, 1), "parts12": (1, 2), "parts33": (3, 3)}[what]
        pic, ns, tg = _new_pic(rng, w, h, bd, cf, nrefs=3, target=1)
        shapes = [(16, ["P"] * 4), (8, ["P"] * 4), (4, ["P"] * 4), (16, ["B"] * 4), (8, ["B"] * 4), (4, ["B"] * 4),
                  (8, ["0", "1", "1", "0"]), (4, ["1", "0", "B", "1"]), (8, ["B", "0", "1", "B"])]
        for a in range(w * h):
            gran, lists = shapes[(a + hash_name(what)) % len(shapes)]
            same = a % 3 == 2  # the same slot in both lists
            refs = [[int(rng.choice([0, 2, 3])) for _ in range(4)] for _ in range(2)]
            if gran == 16:
                refs = [[refs[0][0]] * 4, [refs[1][0]] * 4]
            if same:
                refs[1] = list(refs[0])
            tab = rng.integers(-30, 31, size=(2, 4, 4, 2))
            t8 = bool(a & 1)
            pic["mbs"][a] = inter_mb(lambda li, b8, sb, tab=tab: (int(tab[li, b8, sb, 0]), int(tab[li, b8, sb, 1])), gran, lists, refs, t8=t8)
            _residual(rng, pic["mbs"][a], bd, cf, ("mixed", "full", "limit", "none", "chroma")[a % 5])
    elif what.startswith("wp"):  # weights: 3 x 3, every MB another flavour
        pic, ns, tg = _new_pic(rng, 3, 3, bd, cf)
        kind = what[2:]  # uni | bi | implicit
        for a in range(9):
            lists = {"uni": ["P", "P", "P", "P"] if a % 2 else ["0", "1", "1", "0"], "bi": ["B"] * 4,
                     "implicit": ["B"] * 4, "mix": ["B", "0", "1", "B"]}[kind]
            ws = []
            for b8 in range(4):
                bi = lists[b8] == "B"
                if kind == "implicit":
                    ws.append(_weight(rng, "implicit", True))
                elif a == 0:  # clips at both ends whatever the samples
                    ws.append(_weight(rng, ("fixed", 0, 127, 0 if bi else 127, 127, 127), bi) if b8 % 2 else
                              _weight(rng, ("fixed", 0, -128, 0 if bi else -128, -128, -128), bi))
                elif a == 1:  # the rounding terms alone: weight 1 at every logWD, no offset
                    lwd = (0, 1, 5, 7)[b8]
                    one = 1 << lwd
                    ws.append(_weight(rng, ("fixed", lwd, one // 2 + 1, one // 2, 1, 0), True) if bi else
                              _weight(rng, ("fixed", lwd, one, one, 0, 0), False))
                else:
                    ws.append(_weight(rng, "explicit", bi))
            tab = rng.integers(-20, 21, size=(2, 4, 2))
            pic["mbs"][a] = inter_mb(lambda li, b8, sb, tab=tab: (int(tab[li, b8, 0]), int(tab[li, b8, 1])), 8, lists,
                                     [[0, 1, 0, 1], [1, 0, 0, 1]], weights=ws, t8=a == 4)
            _residual(rng, pic["mbs"][a], bd, cf, "none" if a < 6 else "sparse")
        expect = {"clips": kind != "implicit"}
    elif what.startswith("field"):  # field pictures referencing fields of both parities (chroma offset)
        f = int(what[-1])
        pic, ns, tg = _new_pic(rng, 2, 2, bd, cf, nrefs=4, field=f, target=4 if f == 1 else 3)
        others = [s for s in range(ns) if s != tg]
        for a in range(4):
            tab = rng.integers(-40, 41, size=(2, 4, 4, 2))
            refs = [[others[(a + b8) % 4] for b8 in range(4)], [others[(a + b8 + 1) % 4] for b8 in range(4)]]
            pic["mbs"][a] = inter_mb(lambda li, b8, sb, tab=tab: (int(tab[li, b8, sb, 0]), int(tab[li, b8, sb, 1])), 4, ["B", "0", "1", "B"], refs)
            _residual(rng, pic["mbs"][a], bd, cf, "sparse")
    else:
        raise KeyError(name)
    return _finish(name, pic, ns, tg, rng, expect)


INTRA_KINDS = ("i4", "i8", "i16")


def mixed_picture(name, wmbs, hmbs, bd, cf, seed, nslices=1, constrained=False, p_intra=1.0, slice_offset=0, how="mixed"):
    """Random MB types: intra with probability p_intra, else I_PCM / zero-vector skip / a small
    inter MB; slices cut at arbitrary addresses."""
    rng = np.random.default_rng(seed)
    pic, ns, tg = _new_pic(rng, wmbs, hmbs, bd, cf, nrefs=1, constrained=constrained)
    sl = _slices_by_rows(wmbs, hmbs, nslices, slice_offset)
    kinds = []
    for a in range(wmbs * hmbs):
        k = str(rng.choice(INTRA_KINDS)) if rng.random() < p_intra else str(rng.choice(["pcm", "skip", "inter"]))
        kinds.append(k)
        pic["mbs"][a] = {"type": "inter" if k in ("skip", "inter") else k, "slice": sl[a]}
    for a, k in enumerate(kinds):
        if k == "pcm":
            pic["mbs"][a] = pcm_mb(rng, bd, cf, sl[a])
        elif k == "skip":
            pic["mbs"][a] = skip_mb(0, sl[a])
        elif k == "inter":
            v = (int(rng.integers(-8, 9)) * 4, int(rng.integers(-8, 9)) * 4)
            pic["mbs"][a] = inter_mb(lambda li, b8, sb, v=v: v, 16, ["P"] * 4, [[0] * 4, [0] * 4], slice_=sl[a])
            _residual(rng, pic["mbs"][a], bd, cf, "sparse")
        else:
            intra_mb(rng, pic, a, k, bd, cf, how)
    return _finish(name, pic, ns, tg, rng)


def structure_picture(name, wmbs, hmbs, bd, cf, seed):
    """Mostly I_PCM and zero-vector skips (cheap for the oracle); intra MBs where the intra
    wavefront's structure is: around the 64-MB chunk edges of a row, in the first and last row of
    each eight-row group, in runs (left column carried in LDS) and alone (left column from the
    picture)."""
    rng = np.random.default_rng(seed)
    pic, ns, tg = _new_pic(rng, wmbs, hmbs, bd, cf, nrefs=1)
    cols = {c for base in range(0, wmbs + 64, 64) for c in (base - 2, base - 1, base, base + 1, base + 63, base + 64)}
    cols |= {3, 4, 5, 8, wmbs - 1, 239, 240}
    rows = {0, 1, 7, 8, 9, 15, 16, hmbs - 1}
    n = wmbs * hmbs
    intra = [(a % wmbs) in cols and (a // wmbs) in rows for a in range(n)]
    if n <= 40:
        intra = [rng.random() < 0.7 for _ in range(n)]
    for a in range(n):
        pic["mbs"][a] = {"type": "i4" if intra[a] else ("pcm" if rng.integers(0, 4) else "inter"), "slice": 0}
    for a in range(n):
        if intra[a]:
            intra_mb(rng, pic, a, str(rng.choice(INTRA_KINDS)), bd, cf, "sparse")
        elif pic["mbs"][a]["type"] == "pcm":
            pic["mbs"][a] = pcm_mb(rng, bd, cf)
        else:
            pic["mbs"][a] = skip_mb(0)
    return _finish(name, pic, ns, tg, rng)


INTER_NAMES = ["inter_frac", "inter_far", "inter_edge", "inter_parts11", "inter_parts21", "inter_parts12", "inter_parts33",
               "inter_wpuni", "inter_wpbi", "inter_wpimplicit", "inter_wpmix"]
FIELD_NAMES = ["inter_field1", "inter_field2"]  # 8-bit 4:2:0 only: the parser refuses other field pictures
AVAIL_NAMES = ["avail_slices3", "avail_constrained", "avail_constrained_b", "avail_constrained_c", "avail_constrained_e", "avail_constrained_f",
               "avail_constrained_slices",
               "dense_1slice"]
STRUCT_NAMES = [f"wide_{w}x{h}" for w in WIDE for h in (2, 9)] + [f"tall_{w}x{h}" for h in TALL for w in ((1, 3) if h % 2 else (2, 5))]
HBD_NAMES = [f"shape_{w}x{h}" for w, h in HBD_SHAPES]
_CACHE = {}


def case_names(bd, cf):
    names = INTER_NAMES + AVAIL_NAMES + HBD_NAMES
    if (bd, cf) == (8, 1):
        names = names + FIELD_NAMES + STRUCT_NAMES
    return names


def get_case(name, bd=8, cf=1):
    key = (name, bd, cf)
    if key in _CACHE:
        return _CACHE[key]
    seed = _seed(name, bd, cf)
    if name.startswith("inter_"):
        c = inter_case(name, bd, cf)
    elif name == "avail_slices3":
        c = mixed_picture(name, 17, 9, bd, cf, seed, nslices=3, slice_offset=5)
    elif name.startswith("avail_constrained") and not name.endswith("slices"):
        c = mixed_picture(name, 17, 9, bd, cf, seed, constrained=True, p_intra={"d": 0.55, "b": 0.4, "c": 0.7, "e": 0.5, "f": 0.6}[name[-1]])
    elif name == "avail_constrained_slices":
        c = mixed_picture(name, 9, 9, bd, cf, seed, nslices=4, slice_offset=3, constrained=True, p_intra=0.6)
    elif name == "dense_1slice":
        c = mixed_picture(name, 17, 9, bd, cf, seed)
    elif name.startswith("shape_") or name.startswith("many_"):
        w, h = (int(v) for v in name.split("_")[1].split("x"))
        c = mixed_picture(name, w, h, bd, cf, seed, nslices=1 + (w * h > 20), slice_offset=2, p_intra=0.7,
                          constrained=name.startswith("many_") and h == 9, how="sparse" if w * h > 200 else "mixed")
    elif name.startswith("wide_") or name.startswith("tall_"):
        w, h = (int(v) for v in name.split("_")[1].split("x"))
        c = structure_picture(name, w, h, bd, cf, seed)
    else:
        raise KeyError(name)
    _CACHE[key] = c
    return c


def many_names():
    return [f"many_{w}x{h}_{i}" for i, (w, h) in enumerate(zip(MANY_WIDTHS, MANY_HEIGHTS))]


def oracle(case):
    """(y, cb, cr, stats) of the oracle, once per case; case['oracle_s'] = its time."""
    if "_oracle" not in case:
        t0 = time.perf_counter()
        case["_oracle"] = ro.reconstruct_picture(case["pic"], *case["init"])
        case["oracle_s"] = time.perf_counter() - t0
    return case["_oracle"]


def run_native(native, case, device=-1):
    return split(native.avc_recon_records(device=device, **case["args"]))


def split(out):
    """(y, interleaved uv) -> (y, cb, cr)."""
    y, uv = out
    return y, uv[:, 0::2], uv[:, 1::2]


def explain(case, got, want):
    return ro.explain(case["pic"], got, want)


def check_honest(case):
    """The case does what its name says, judged from the oracle's own statistics."""
    st = oracle(case)[3]
    ex = case["expect"]
    for side in ex.get("clamp", []):
        assert st["clamp"][side] > 0, f"{case['name']}: no reference fetch clamped at the {side} edge"
    if ex.get("clips"):
        assert st["clip0"] > 0 and st["clipmax"] > 0, f"{case['name']}: weighted samples clipped {st['clip0']} / {st['clipmax']}"
    if ex.get("frac"):
        assert len(st["luma_frac"]) == 16, f"{case['name']}: luma positions {sorted(st['luma_frac'])}"
        want = 64 if case["pic"]["cf"] == 1 else 32  # (4:2:2: yFracC = (mvy & 3) << 1 is even)
        assert len(st["chroma_frac"]) == want, f"{case['name']}: {len(st['chroma_frac'])} chroma positions"


def allowed_intra_pairs():
    """Every (kind, mode, availability) the standard allows: block modes by (left, top, top-left),
    MB modes by (A, B, D)."""
    out = set()
    for left in (False, True):
        for top in (False, True):
            for tl in (False, True):
                for kind, table in (("i4", ro._NEEDS), ("i8", ro._NEEDS)):
                    out |= {(kind, m, left, top, tl) for m in ro.allowed_modes(table, top, left, tl)}
                out |= {("i16", m, left, top, tl) for m in ro.allowed_modes(ro._NEEDS16, top, left, tl)}
                out |= {("chroma", m, left, top, tl) for m in ro.allowed_modes(ro._NEEDSC, top, left, tl)}
    return out


def intra_pairs_hit(cases):
    hit, kinds = set(), set()
    for c in cases:
        st = oracle(c)[3]
        for e in st["intra"]:
            hit.add((e[0], e[1], e[2], e[3], e[5]) if e[0] in ("i4", "i8") else e)
        kinds |= st["kinds"]
    return hit, kinds
