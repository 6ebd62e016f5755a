"""Whole-picture H.264 reconstruction oracle (inter prediction, intra prediction, residual, I_PCM;
no loop filter), written from the text of ITU-T H.264 (2016) on top of the per-block functions of
spec_oracle.py. It imports nothing of the package and knows nothing of the decoder's record
layout: a picture is a dict, a macroblock is a dict, a reference picture is named by any key.

picture = {
  "wmbs", "hmbs", "bd" (8..10), "cf" (chroma_format_idc 1 or 2),
  "field": 0 frame, 1 top field, 2 bottom field picture (field_pic_flag, bottom_field_flag),
  "constrained": constrained_intra_pred_flag,
  "refs": {name: {"y": 2-D array, "cb": ..., "cr": ..., "bottom": bool (field parity)}},
  "mbs": [macroblock, ...] in raster order }

macroblock = {"type": "inter" | "pcm" | "i4" | "i8" | "i16", "slice": int, ...}
  inter: "parts": four 8x8 partitions (raster), each {"l0": None | (ref name, [four (mvx, mvy), one
         per 4x4 sub-block, raster in the 8x8]), "l1": the same, "w": None (default weighted
         prediction) | three per-component dicts {"lwd", "w0", "w1", "o0", "o1"} with the offsets as
         the syntax elements give them (8.4.2.3.2 scales them by 1 << (BitDepth - 8))}
  pcm:   "y" (16x16), "cb", "cr" (MbHeightC x 8) sample arrays
  i4:    "modes": 16 Intra4x4PredMode by raster 4x4 block; i8: "modes": 4 Intra8x8PredMode by raster
         8x8 block; i16: "mode": Intra16x16PredMode; all three: "cmode": intra_chroma_pred_mode
  all but pcm: "t8": transform_size_8x8_flag, "luma": {raster 4x4 block (t8: raster 8x8 block):
         rows of scaled coefficients d_ij}, "chroma": {(component 0 / 1, raster 4x4 block, 2 wide):
         4x4 rows}; the coefficients are the inverse transform's input (dequantised already).
"""
from __future__ import annotations

import numpy as np

import spec_oracle as so

NA = -(10 ** 9)  # poison for samples "marked as not available for Intra prediction"


# ------------------------------------------------------------------ 8.4.2.3 weighted prediction
def weighted_default(p0, p1):
    """8.4.2.3.1: one list's sample, or (predPartL0 + predPartL1 + 1) >> 1. None = list unused."""
    if p0 is not None and p1 is not None:
        return (p0 + p1 + 1) >> 1
    return p0 if p0 is not None else p1


def weighted_unclipped(p0, p1, lwd, w0, w1, o0, o1):
    """The argument of Clip1 in 8-297 .. 8-299."""
    if p0 is not None and p1 is not None:
        return ((p0 * w0 + p1 * w1 + 2 ** lwd) >> (lwd + 1)) + ((o0 + o1 + 1) >> 1)
    p, w, o = (p0, w0, o0) if p0 is not None else (p1, w1, o1)
    return ((p * w + 2 ** (lwd - 1)) >> lwd) + o if lwd >= 1 else p * w + o


def weighted_explicit(p0, p1, lwd, w0, w1, o0, o1, bd=8):
    """8.4.2.3.2 (8-297 .. 8-299): o0 / o1 are the values already scaled to the bit depth (explicit:
    offset << (BitDepth - 8); implicit: 0). Single list: the used list's p / w / o."""
    return so.clip1(weighted_unclipped(p0, p1, lwd, w0, w1, o0, o1), bd)


# ------------------------------------------------------------------ 8.4.1.4 / 8.4.2.2.2 chroma vectors
def chroma_vector(mvx, mvy, cf, cur_bottom=None, ref_bottom=None):
    """Luma vector (quarter luma samples) -> ((xInt offset, xFracC), (yInt offset, yFracC)) of the
    chroma vector, fractions in eighths. The chroma vector has units of 1 / (4 SubWidthC) and 1 /
    (4 SubHeightC) chroma samples. cur_bottom / ref_bottom: for a field (macroblock) only, the
    parities of the current and the referenced field: Table 8-9 offsets the vertical component by
    -2 (reference bottom, current top) or +2 (reference top, current bottom), ChromaArrayType 1
    only."""
    sub_w, sub_h = 2, (2 if cf == 1 else 1)
    if cur_bottom is not None and cf == 1:
        if ref_bottom and not cur_bottom:
            mvy -= 2
        elif not ref_bottom and cur_bottom:
            mvy += 2
    ex = mvx * 8 // (4 * sub_w)  # in eighths of a chroma sample (exact: 8 / (4 Sub) is 1 or 2)
    ey = mvy * 8 // (4 * sub_h)
    return (ex // 8, ex % 8), (ey // 8, ey % 8)  # (floor division: the standard's >> and &)


# ------------------------------------------------------------------ 8.5.12.2 / 8.5.13.2 with the range rule
def _in_range(vals, bd, what):
    lo, hi = -(1 << (7 + bd)), (1 << (7 + bd)) - 1
    for v in vals:
        assert lo <= v <= hi, f"{what} {v} outside {lo}..{hi}: not a conforming stream (8.5.12.2 / 8.5.13.2)"


def residual_4x4(d, bd):
    """inverse_4x4 with the bitstream constraint of 8.5.12.2 on d, e, f, g, h asserted."""
    _in_range([v for row in d for v in row], bd, "d")
    f = []
    for i in range(4):
        e = [d[i][0] + d[i][2], d[i][0] - d[i][2], (d[i][1] >> 1) - d[i][3], d[i][1] + (d[i][3] >> 1)]
        f.append([e[0] + e[3], e[1] + e[2], e[1] - e[2], e[0] - e[3]])
        _in_range(e + f[-1], bd, "e/f")
    for j in range(4):
        g = [f[0][j] + f[2][j], f[0][j] - f[2][j], (f[1][j] >> 1) - f[3][j], f[1][j] + (f[3][j] >> 1)]
        _in_range(g + [g[0] + g[3], g[1] + g[2], g[1] - g[2], g[0] - g[3]], bd, "g/h")
    return so.inverse_4x4(d)


def _t8_values(v):
    """Every intermediate of one 8.5.13.2 pass (the a / b values), for the range rule."""
    e = [v[0] + v[4], -v[3] + v[5] - v[7] - (v[7] >> 1), v[0] - v[4], v[1] + v[7] - v[3] - (v[3] >> 1),
         (v[2] >> 1) - v[6], -v[1] + v[7] + v[5] + (v[5] >> 1), v[2] + (v[6] >> 1), v[3] + v[5] + v[1] + (v[1] >> 1)]
    f = [e[0] + e[6], e[1] + (e[7] >> 2), e[2] + e[4], e[3] + (e[5] >> 2), e[2] - e[4], (e[3] >> 2) - e[5],
         e[0] - e[6], e[7] - (e[1] >> 2)]
    g = [f[0] + f[7], f[2] + f[5], f[4] + f[3], f[6] + f[1], f[6] - f[1], f[4] - f[3], f[2] - f[5], f[0] - f[7]]
    return e + f + g, g


def residual_8x8(d, bd):
    _in_range([v for row in d for v in row], bd, "d")
    rows = []
    for i in range(8):
        allv, g = _t8_values(d[i])
        _in_range(allv, bd, "8x8 row pass")
        rows.append(g)
    for j in range(8):
        allv, _ = _t8_values([rows[i][j] for i in range(8)])
        _in_range(allv, bd, "8x8 column pass")
    return so.inverse_8x8(d)


# ------------------------------------------------------------------ 6.4.3 / 6.4.11 / 6.4.12 neighbours
def blk4_xy(idx):
    """6.4.3: upper-left luma sample of 4x4 luma block luma4x4BlkIdx."""
    return (idx // 4 % 2) * 8 + (idx % 4 % 2) * 4, (idx // 4 // 2) * 8 + (idx % 4 // 2) * 4


def blk4_idx(x, y):
    for idx in range(16):
        bx, by = blk4_xy(idx)
        if bx <= x < bx + 4 and by <= y < by + 4:
            return idx
    raise ValueError((x, y))


def mb_neighbours(pic, addr):
    """6.4.9 / 6.4.11.1 (MbaffFrameFlag 0): mbAddrA / B / C / D, None where not available: outside
    the picture, in another slice (or later in decoding order)."""
    w = pic["wmbs"]
    mbs = pic["mbs"]

    def ok(n, edge):
        return n if (n >= 0 and not edge and mbs[n]["slice"] == mbs[addr]["slice"]) else None

    return {"A": ok(addr - 1, addr % w == 0), "B": ok(addr - w, False), "C": ok(addr - w + 1, (addr + 1) % w == 0),
            "D": ok(addr - w - 1, addr % w == 0)}


def intra_usable(pic, n):
    """8.3.1.2 / 8.3.2.2 / 8.3.3 / 8.3.4: samples of mbAddrN are not available for Intra prediction
    when it is not available, or is coded in Inter prediction mode with constrained_intra_pred."""
    if n is None:
        return False
    return not (pic["constrained"] and pic["mbs"][n]["type"] == "inter")


def locate(nb, xn, yn):
    """6.4.12: which macroblock covers luma location (xN, yN) relative to the current MB's corner."""
    if yn > 15 or (xn > 15 and yn >= 0):
        return None
    if yn < 0:
        return "D" if xn < 0 else ("B" if xn <= 15 else "C")
    return "A" if xn < 0 else "cur"


# ------------------------------------------------------------------ the picture
def new_stats():
    return {"luma_frac": set(), "chroma_frac": set(), "clamp": {"left": 0, "right": 0, "top": 0, "bottom": 0},
            "clip0": 0, "clipmax": 0, "intra": set(), "kinds": set()}


def _count_clamp(st, x0, x1, y0, y1, w, h):
    c = st["clamp"]
    c["left"] += x0 < 0
    c["right"] += x1 > w - 1
    c["top"] += y0 < 0
    c["bottom"] += y1 > h - 1


def _lists(ref):
    if "_l" not in ref:
        ref["_l"] = tuple(np.asarray(ref[k]).tolist() for k in ("y", "cb", "cr"))
    return ref["_l"]


def _pred_block(pic, ref, comp, x0, y0, bw, bh, ix, fx, iy, fy, st):
    """One list's prediction of a bw x bh block of component comp (0 luma) whose first sample is at
    (x0, y0): 8.4.2.2.1 / 8.4.2.2.2 per sample; a vector without fraction is the clamped copy that
    both reduce to for xFrac = yFrac = 0."""
    plane = np.asarray(ref[("y", "cb", "cr")[comp]])
    h, w = plane.shape
    reach = (2, 3) if comp == 0 else (0, 1)
    _count_clamp(st, x0 + ix - (reach[0] if fx else 0), x0 + ix + bw - 1 + (reach[1] if fx else 0),
                 y0 + iy - (reach[0] if fy else 0), y0 + iy + bh - 1 + (reach[1] if fy else 0), w, h)
    if fx == 0 and fy == 0:
        ys = np.clip(np.arange(y0 + iy, y0 + iy + bh), 0, h - 1)
        xs = np.clip(np.arange(x0 + ix, x0 + ix + bw), 0, w - 1)
        return plane[np.ix_(ys, xs)].astype(np.int64).tolist()
    rows = _lists(ref)[comp]
    if comp == 0:
        return [[so.luma_sample(rows, x0 + ix + x, y0 + iy + y, fx, fy, pic["bd"]) for x in range(bw)] for y in range(bh)]
    return [[so.chroma_sample(rows, x0 + ix + x, y0 + iy + y, fx, fy) for x in range(bw)] for y in range(bh)]


def _inter_mb(pic, mb, mx, my, planes, st):
    bd, cf = pic["bd"], pic["cf"]
    sub_h = 2 if cf == 1 else 1
    cur_bottom = None if not pic["field"] else pic["field"] == 2
    for b8, part in enumerate(mb["parts"]):
        for sb in range(4):  # 4x4 sub-blocks: the smallest sub-macroblock partition
            lx, ly = (b8 % 2) * 8 + (sb % 2) * 4, (b8 // 2) * 8 + (sb // 2) * 4
            for comp in range(3):
                if comp == 0:
                    bw, bh, x0, y0 = 4, 4, mx * 16 + lx, my * 16 + ly
                else:
                    bw, bh = 2, 4 // sub_h
                    x0, y0 = mx * 8 + lx // 2, my * (16 // sub_h) + ly // sub_h
                preds = []
                for lst in ("l0", "l1"):
                    if part[lst] is None:
                        preds.append(None)
                        continue
                    name, mvs = part[lst]
                    ref = pic["refs"][name]
                    mvx, mvy = mvs[sb]
                    if comp == 0:
                        ix, fx, iy, fy = mvx >> 2, mvx & 3, mvy >> 2, mvy & 3  # (8-225 .. 8-228)
                        st["luma_frac"].add((fx, fy))
                    else:
                        (ix, fx), (iy, fy) = chroma_vector(mvx, mvy, cf, cur_bottom,
                                                           None if cur_bottom is None else ref["bottom"])
                        st["chroma_frac"].add((fx, fy))
                    preds.append(_pred_block(pic, ref, comp, x0, y0, bw, bh, ix, fx, iy, fy, st))
                assert preds[0] is not None or preds[1] is not None, "partition without a reference"
                w = part["w"]
                for y in range(bh):
                    for x in range(bw):
                        p0 = None if preds[0] is None else preds[0][y][x]
                        p1 = None if preds[1] is None else preds[1][y][x]
                        if w is None:
                            v = weighted_default(p0, p1)
                        else:
                            e = w[comp]
                            sc = 1 << (bd - 8)  # (8.4.2.3.2: o = offset << (BitDepth - 8))
                            raw = weighted_unclipped(p0, p1, e["lwd"], e["w0"], e["w1"], e["o0"] * sc, e["o1"] * sc)
                            v = so.clip1(raw, bd)
                            st["clip0"] += raw < 0
                            st["clipmax"] += raw > (1 << bd) - 1
                        planes[comp][y0 + y][x0 + x] = v
    st["kinds"].add(("inter", mb.get("t8", False)))
    _add_residual(pic, mb, mx, my, planes)


def _add_residual(pic, mb, mx, my, planes, luma=True):
    """8.5.14: u = Clip1(pred + r) over the prediction already in `planes` (inter MBs and the
    chroma of intra MBs; intra luma adds its residual block by block)."""
    bd = pic["bd"]
    if luma:
        n = 8 if mb.get("t8") else 4
        for blk, d in mb.get("luma", {}).items():
            r = residual_8x8(d, bd) if n == 8 else residual_4x4(d, bd)
            x0, y0 = mx * 16 + (blk % (16 // n)) * n, my * 16 + (blk // (16 // n)) * n
            for y in range(n):
                for x in range(n):
                    planes[0][y0 + y][x0 + x] = so.clip1(int(planes[0][y0 + y][x0 + x]) + r[y][x], bd)
    hc = 8 if pic["cf"] == 1 else 16
    for (c, blk), d in mb.get("chroma", {}).items():
        r = residual_4x4(d, bd)
        x0, y0 = mx * 8 + (blk % 2) * 4, my * hc + (blk // 2) * 4
        for y in range(4):
            for x in range(4):
                planes[1 + c][y0 + y][x0 + x] = so.clip1(int(planes[1 + c][y0 + y][x0 + x]) + r[y][x], bd)


_NEEDS = {  # which neighbours a mode reads: (top, left, top-left), 8.3.1.2.x / 8.3.2.2.x
    0: (1, 0, 0), 1: (0, 1, 0), 2: (0, 0, 0), 3: (1, 0, 0), 4: (1, 1, 1), 5: (1, 1, 1), 6: (1, 1, 1), 7: (1, 0, 0),
    8: (0, 1, 0)}
_NEEDS16 = {0: (1, 0, 0), 1: (0, 1, 0), 2: (0, 0, 0), 3: (1, 1, 1)}      # Intra16x16PredMode
_NEEDSC = {0: (0, 0, 0), 1: (0, 1, 0), 2: (1, 0, 0), 3: (1, 1, 1)}       # intra_chroma_pred_mode


def allowed_modes(table, has_top, has_left, has_tl):
    return [m for m, (t, l, d) in table.items() if (not t or has_top) and (not l or has_left) and (not d or has_tl)]


def block_availability(pic, addr, bx, by):
    """(has_top, has_left, has_top_left) of the luma block whose corner is (bx, by) in MB addr, by
    6.4.12: neighbours inside the MB precede the block in decoding order."""
    nb = mb_neighbours(pic, addr)

    def ok(xn, yn):
        where = locate(nb, xn, yn)
        return where == "cur" or (where is not None and intra_usable(pic, nb[where]))

    return ok(bx, by - 1), ok(bx - 1, by), ok(bx - 1, by - 1)


def _intra_luma_nxn(pic, mb, addr, mx, my, Y, st, n):
    """Intra_4x4 (n = 4, 8.3.1.2) / Intra_8x8 (n = 8, 8.3.2.2): block by block in decoding order,
    each predicted from the constructed samples around it, then its residual added."""
    bd = pic["bd"]
    nb = mb_neighbours(pic, addr)
    usable = {k: intra_usable(pic, v) for k, v in nb.items()}
    order = [blk4_xy(i) for i in range(16)] if n == 4 else [((i % 2) * 8, (i // 2) * 8) for i in range(4)]
    done = set()  # upper-left corners of the blocks of this MB decoded so far

    def sample(xn, yn):  # p at luma location (xn, yn) relative to the MB, NA if not available
        where = locate(nb, xn, yn)
        if where is None:
            return NA
        if where == "cur":
            return int(Y[my * 16 + yn][mx * 16 + xn]) if (xn // n * n, yn // n * n) in done else NA
        return int(Y[my * 16 + yn][mx * 16 + xn]) if usable[where] else NA

    for bx, by in order:
        raster = (by // n) * (16 // n) + bx // n
        mode = mb["modes"][raster]
        top = [sample(bx + x, by - 1) for x in range(-1, 2 * n)]
        left = [sample(bx - 1, by + y) for y in range(n)]
        has_top, has_left, has_tl, has_tr = top[1] != NA, left[0] != NA, top[0] != NA, top[n + 1] != NA
        if has_top and not has_tr:  # "substituted by p[n - 1, -1]"
            top[n + 1:] = [top[n]] * n
        assert mode in allowed_modes(_NEEDS, has_top, has_left, has_tl), \
            f"MB {addr} block ({bx},{by}): mode {mode} reads samples that are not available"
        st["intra"].add(("i4" if n == 4 else "i8", mode, has_left, has_top, has_tr, has_tl))
        if n == 4:
            pred = so.intra_4x4(top, left, has_top, has_left, mode, bd)
        else:
            pred = so.intra_8x8(top, left, has_top, has_left, has_tl, mode, bd)
        d = mb.get("luma", {}).get(raster)
        r = None if d is None else (residual_4x4(d, bd) if n == 4 else residual_8x8(d, bd))
        for y in range(n):
            for x in range(n):
                Y[my * 16 + by + y][mx * 16 + bx + x] = so.clip1(pred[y][x] + (r[y][x] if r else 0), bd)
        done.add((bx, by))


def _intra_mb(pic, mb, addr, mx, my, planes, st):
    bd, cf = pic["bd"], pic["cf"]
    nb = mb_neighbours(pic, addr)
    A, B, C, D = (intra_usable(pic, nb[k]) for k in "ABCD")
    st["kinds"].add((mb["type"], A, B, C, D))
    Y = planes[0]
    if mb["type"] == "i16":
        top = [int(Y[my * 16 - 1][mx * 16 + x]) if (B if x >= 0 else D) else NA for x in range(-1, 16)]
        left = [int(Y[my * 16 + y][mx * 16 - 1]) if A else NA for y in range(16)]
        assert mb["mode"] in allowed_modes(_NEEDS16, B, A, D), f"MB {addr}: Intra_16x16 mode {mb['mode']} not allowed"
        st["intra"].add(("i16", mb["mode"], A, B, D))
        pred = so.intra_16x16(top, left, B, A, mb["mode"], bd)
        for y in range(16):
            for x in range(16):
                Y[my * 16 + y][mx * 16 + x] = pred[y][x]
        _add_residual(pic, {"luma": mb.get("luma", {}), "t8": False}, mx, my, planes)
    else:
        _intra_luma_nxn(pic, mb, addr, mx, my, Y, st, 4 if mb["type"] == "i4" else 8)
    hc = 8 if cf == 1 else 16
    assert mb["cmode"] in allowed_modes(_NEEDSC, B, A, D), f"MB {addr}: chroma mode {mb['cmode']} not allowed"
    st["intra"].add(("chroma", mb["cmode"], A, B, D))
    for c in (1, 2):
        P = planes[c]
        top = [int(P[my * hc - 1][mx * 8 + x]) if (B if x >= 0 else D) else NA for x in range(-1, 8)]
        left = [int(P[my * hc + y][mx * 8 - 1]) if A else NA for y in range(hc)]
        pred = so.intra_chroma(top, left, B, A, mb["cmode"], bd, cf)
        for y in range(hc):
            for x in range(8):
                P[my * hc + y][mx * 8 + x] = pred[y][x]
    _add_residual(pic, {"chroma": mb.get("chroma", {})}, mx, my, planes, luma=False)


def reconstruct_picture(pic, y, cb, cr):
    """The decoding process of 8.3 - 8.5 over the macroblocks in address order, into copies of the
    given planes (the target's previous contents: every sample is overwritten). Returns (y, cb, cr,
    stats)."""
    planes = [np.array(p, dtype=np.int64) for p in (y, cb, cr)]
    st = new_stats()
    w, hc = pic["wmbs"], 8 if pic["cf"] == 1 else 16
    for addr, mb in enumerate(pic["mbs"]):
        mx, my = addr % w, addr // w
        if mb["type"] == "pcm":  # 8.3.5: the samples as sent
            planes[0][my * 16:my * 16 + 16, mx * 16:mx * 16 + 16] = mb["y"]
            planes[1][my * hc:my * hc + hc, mx * 8:mx * 8 + 8] = mb["cb"]
            planes[2][my * hc:my * hc + hc, mx * 8:mx * 8 + 8] = mb["cr"]
            st["kinds"].add(("pcm",))
        elif mb["type"] == "inter":
            _inter_mb(pic, mb, mx, my, planes, st)
        else:
            _intra_mb(pic, mb, addr, mx, my, planes, st)
    return planes[0], planes[1], planes[2], st


def describe_mb(pic, addr):
    mb = pic["mbs"][addr]
    t = mb["type"]
    s = f"MB {addr} ({addr % pic['wmbs']}, {addr // pic['wmbs']}) slice {mb['slice']} {t}"
    if t == "inter":
        s += " parts " + "; ".join(
            f"l0 {p['l0']} l1 {p['l1']} w {'default' if p['w'] is None else p['w']}" for p in mb["parts"])
    elif t in ("i4", "i8"):
        s += f" modes {mb['modes']} chroma mode {mb['cmode']}"
    elif t == "i16":
        s += f" mode {mb['mode']} chroma mode {mb['cmode']}"
    if t != "pcm":
        nb = mb_neighbours(pic, addr)
        s += " usable A/B/C/D " + "/".join(str(int(intra_usable(pic, nb[k]))) for k in "ABCD")
        s += f" t8 {int(bool(mb.get('t8')))} coded luma {sorted(mb.get('luma', {}))} chroma {sorted(mb.get('chroma', {}))}"
    return s


def explain(pic, got, want):
    """None if the planes agree; else the first differing macroblock in decoding order: its kind,
    modes and neighbours, the plane, the 4x4 block and the sample. got / want: (y, cb, cr)."""
    w, hc = pic["wmbs"], 8 if pic["cf"] == 1 else 16
    diffs = [np.asarray(g).astype(np.int64) != np.asarray(e) for g, e in zip(got, want)]
    if not any(d.any() for d in diffs):
        return None
    for addr in range(len(pic["mbs"])):
        mx, my = addr % w, addr // w
        for c, (bw, bh) in enumerate(((16, 16), (8, hc), (8, hc))):
            blk = diffs[c][my * bh:(my + 1) * bh, mx * bw:(mx + 1) * bw]
            if blk.any():
                yy, xx = (int(v[0]) for v in np.nonzero(blk))
                g = int(np.asarray(got[c])[my * bh + yy][mx * bw + xx])
                e = int(np.asarray(want[c])[my * bh + yy][mx * bw + xx])
                return (f"{('luma', 'Cb', 'Cr')[c]} sample ({xx}, {yy}) of 4x4 block {(yy // 4) * (bw // 4) + xx // 4} "
                        f"(raster) is {g}, expected {e}; {int(blk.sum())} samples of the MB differ, "
                        f"{int(sum(d.sum() for d in diffs))} of the picture; {describe_mb(pic, addr)}")
    raise AssertionError("unreachable")
