"""Seeded pictures for the H.265 loop-filter tests: the state a parser would leave behind
(per 4x4 block intra / cbf / edge flags / QpY / motion, per CTB slice and SAO parameters, slice
headers with reference lists as picture ids, tile layout) together with NV12 planes whose content
makes the filters engage. `records_of` turns such a picture into the records the kernels read,
through the spec oracle's boundary_strengths and the plain meaning of each field - never through
the code under test. `coverage` names, from the oracle's trace alone, what a case reaches; each
case lists what it is for (`reach`) and tests/test_spec_oracle_hevc_lf.py asserts it.

Decisions that the syntax makes per coding unit (intra, QpY, pcm / bypass) are drawn per 8x8
block, the smallest coding unit: a chroma edge section (4 chroma lines = 8 luma lines) then has
one bS 2 decision, one QpY pair and one exemption, as in any stream."""
from __future__ import annotations

import random

import numpy as np

import spec_oracle_hevc as so

EDGE_TU_V, EDGE_TU_H, EDGE_PU_V, EDGE_PU_H = 1, 2, 4, 8  # the binding's `edge` bits


# ----------------------------------------------------------------------------- layout (§6.5.1)
def tile_bounds(total, count, uniform, sizes):
    if uniform:
        return [(i * total) // count for i in range(count + 1)]
    bd = [0]
    for s in sizes:
        bd.append(bd[-1] + s)
    return bd + [total]


def tile_layout(wctb, hctb, cols=1, rows=1, uniform=True, col_width=(), row_height=()):
    """-> (ctb_tile per raster address, raster addresses in tile scan)."""
    cb, rb = tile_bounds(wctb, cols, uniform, col_width), tile_bounds(hctb, rows, uniform, row_height)
    tile, ts2rs = [0] * (wctb * hctb), []
    for ty in range(rows):
        for tx in range(cols):
            for y in range(rb[ty], rb[ty + 1]):
                for x in range(cb[tx], cb[tx + 1]):
                    tile[y * wctb + x] = ty * cols + tx
                    ts2rs.append(y * wctb + x)
    return tile, ts2rs


def stride_of(width):
    return (width + 15) // 16 * 16


PAD = 77  # the pitch padding right of the picture: must come back untouched


# ----------------------------------------------------------------------------- plane content
def make_planes(rnd, w, h, bd):
    """Smooth 8x8 blocks (flat, or a ramp, with noise of 0..2) with steps between them, some
    near 0 and near the maximum: like _edge_lines in test_spec_oracle_hevc.py, as a picture."""
    mx, sc = (1 << bd) - 1, 1 << (bd - 8)
    dt = np.uint16 if bd > 8 else np.uint8
    st = stride_of(w)
    y = np.full((h, st), PAD, dt)
    uv = np.full((h // 2, st), PAD, dt)

    def fill(put, bw, bh, n):
        base = rnd.randint(40, 200) * sc
        for by in range(bh):
            for bx in range(bw):
                k = rnd.random()
                if k < 0.12:
                    base = rnd.randint(0, 3)
                elif k < 0.24:
                    base = mx - rnd.randint(0, 3)
                elif k < 0.3:
                    base = rnd.randint(20, 230) * sc
                else:
                    base = so.clip3(0, mx, base + rnd.choice([-30, -12, -6, -3, -2, -1, 0, 0, 1, 2, 3, 6, 12, 30]) * sc)
                gx, gy = rnd.choice([0, 0, 0, 1, -1, 2]), rnd.choice([0, 0, 0, 1, -1])
                noise = rnd.choice([0, 0, 1, 2])
                for j in range(n):
                    for i in range(n):
                        put(bx * n + i, by * n + j, so.clip3(0, mx, base + gx * i + gy * j + rnd.randint(-noise, noise)))

    def put_y(x, yy, v):
        y[yy, x] = v

    fill(put_y, w // 8, h // 8, 8)
    for c in range(2):
        def put_c(x, yy, v, c=c):
            uv[yy, 2 * x + c] = v
        fill(put_c, w // 8, h // 8, 4)
    return y, uv


# ----------------------------------------------------------------------------- pictures
def default_slice(**kw):
    s = dict(ord=0, deblocking_disabled=0, beta_offset_div2=0, tc_offset_div2=0, across_slices=1, sao_luma=1,
             sao_chroma=1, ref_lists=([10, 11, 10], [11, 12]))
    s.update(kw)
    return s


def make_pic(seed, width, height, log2ctb, bd=8, slices=None, starts=(0,), tiles=None, across_tiles=1,
             exempt=True, cqp=(0, 0), sao_eo=None, name=None, reach=()):
    """slices: slice segment dicts (default_slice); starts: each segment's first CTB in tile
    scan; tiles: dict(cols, rows, uniform, col_width, row_height); sao_eo: (luma, chroma) edge
    classes of every CTB, all of type 2 (default: drawn per CTB)."""
    rnd = random.Random(seed)
    w4, h4 = width // 4, height // 4
    n4 = w4 * h4
    ctb = 1 << log2ctb
    wctb, hctb = (width + ctb - 1) // ctb, (height + ctb - 1) // ctb
    t = dict(cols=1, rows=1, uniform=True, col_width=(), row_height=())
    t.update(tiles or {})
    ctb_tile, ts2rs = tile_layout(wctb, hctb, t["cols"], t["rows"], t["uniform"], t["col_width"], t["row_height"])
    slices = [dict(s) for s in (slices or [default_slice()])]
    ctb_slice, ctb_sord = [0] * (wctb * hctb), [0] * (wctb * hctb)
    for ts, rs in enumerate(ts2rs):
        si = max(k for k, s0 in enumerate(starts) if s0 <= ts)
        ctb_slice[rs], ctb_sord[rs] = si, slices[si]["ord"]
    pic = dict(name=name or f"{width}x{height}_ctb{ctb}_bd{bd}_s{seed}", reach=tuple(reach), width=width, height=height,
               log2ctb=log2ctb, bd_y=bd, bd_c=bd, cb_qp_offset=cqp[0], cr_qp_offset=cqp[1],
               pcm_loop_filter_disabled=int(exempt), transquant_bypass=int(exempt), tile_cols=t["cols"], tile_rows=t["rows"],
               uniform_spacing=int(t["uniform"]), col_width=list(t["col_width"]), row_height=list(t["row_height"]),
               across_tiles=across_tiles, slices=slices, ctb_slice=ctb_slice, ctb_sord=ctb_sord, ctb_tile=ctb_tile)
    intra, cbf, qp, pcm, bypass = [0] * n4, [0] * n4, [0] * n4, [0] * n4, [0] * n4
    tu_v, tu_h, pu_v, pu_h = [0] * n4, [0] * n4, [0] * n4, [0] * n4
    mf = [None] * n4
    qlo = -6 * (bd - 8)
    qp_base = rnd.randint(24, 40)
    for y8 in range(height // 8):
        for x8 in range(width // 8):
            sl = slices[ctb_slice[(y8 * 8 >> log2ctb) * wctb + (x8 * 8 >> log2ctb)]]
            is_intra = rnd.random() < 0.25
            k = rnd.random()
            q = so.clip3(qlo, 51, qp_base + rnd.randint(-3, 3) if k < 0.7 else rnd.randint(qlo, 51))
            ex = rnd.random() if exempt else 1.0
            if x8 % 2 == 0 and y8 % 2 == 0 or rnd.random() < 0.4:  # a new motion, else the left / upper block's
                flags = rnd.choice([1, 1, 2, 3, 3])
                l0, l1 = sl["ref_lists"]
                mot = (flags, (rnd.randrange(len(l0)), rnd.randrange(len(l1))),
                       tuple((rnd.choice([0, 0, 3, 4, -4, 7, 16]), rnd.choice([0, 0, 3, 4, -5, 8])) for _ in range(2)))
            elif x8 % 2:
                mot = mf[(y8 * 2) * w4 + x8 * 2 - 1]
            else:
                mot = mf[(y8 * 2 - 1) * w4 + x8 * 2]
            if mot is None or mot[0] == 0 or any(mot[0] >> l & 1 and mot[1][l] >= len(sl["ref_lists"][l]) for l in range(2)):
                mot = (1, (0, 0), ((0, 0), (0, 0)))
            on = [int(rnd.random() < pr) for pr in (0.85, 0.85, 0.5, 0.5)]
            for j in range(2):
                for i in range(2):
                    b = (y8 * 2 + j) * w4 + x8 * 2 + i
                    intra[b], qp[b] = int(is_intra), q
                    pcm[b], bypass[b] = int(ex < 0.05), int(0.05 <= ex < 0.1)
                    cbf[b] = int(rnd.random() < 0.3)
                    mf[b] = (0, (0, 0), ((0, 0), (0, 0))) if is_intra else mot
                    # coding blocks are transform and prediction block edges; inner 4-sample edges
                    # (off the 8x8 grid) exist in the syntax too and must not be filtered
                    # (an edge on the grid runs along the whole 8x8 block)
                    tu_v[b] = on[0] if i == 0 else int(rnd.random() < 0.3)
                    tu_h[b] = on[1] if j == 0 else int(rnd.random() < 0.3)
                    pu_v[b] = on[2] if i == 0 else int(rnd.random() < 0.3)
                    pu_h[b] = on[3] if j == 0 else int(rnd.random() < 0.3)
    pic.update(intra=intra, cbf=cbf, qp=qp, pcm=pcm, bypass=bypass, tu_v=tu_v, tu_h=tu_h, pu_v=pu_v, pu_h=pu_h, mf=mf)
    y, uv = make_planes(rnd, width, height, bd)
    pic.update(y=y, uv=uv)
    # SAO per CTB: the type of Cb serves Cr, as in the syntax; band positions from the CTB's own samples
    lim = (1 << (min(bd, 10) - 5)) - 1
    sao = []
    for ry in range(hctb):
        for rx in range(wctb):
            ty, tc = rnd.choice([0, 1, 2, 2, 2]), rnd.choice([0, 1, 2, 2, 2])
            eo_c = rnd.randrange(4)
            p = dict(type=[ty, tc, tc], band=[0, 0, 0], eo=[rnd.randrange(4), eo_c, eo_c], off=[[0] * 4 for _ in range(3)])
            if sao_eo:
                p.update(type=[2, 2, 2], eo=[sao_eo[0], sao_eo[1], sao_eo[1]])
            for c in range(3):
                sx = min(width - 1, rx * ctb + rnd.randrange(ctb)) >> (c > 0)
                sy = min(height - 1, ry * ctb + rnd.randrange(ctb)) >> (c > 0)
                v = int(y[sy, sx]) if c == 0 else int(uv[sy, 2 * sx + c - 1])
                p["band"][c] = ((v >> (bd - 5)) - rnd.randrange(4)) & 31
                mag = [rnd.choice([lim, lim, rnd.randint(0, lim)]) for _ in range(4)]
                if p["type"][c] == 2:
                    p["off"][c] = [mag[0], mag[1], -mag[2], -mag[3]]
                else:
                    p["off"][c] = [m * rnd.choice([-1, 1]) for m in mag]
            sao.append(p)
    pic["sao"] = sao
    _binding_fields(pic)
    return pic


def _binding_fields(pic):
    """The same motion / edge data in the arrays the binding takes."""
    pic["edge"] = [EDGE_TU_V * a | EDGE_TU_H * b | EDGE_PU_V * c | EDGE_PU_H * d
                   for a, b, c, d in zip(pic["tu_v"], pic["tu_h"], pic["pu_v"], pic["pu_h"])]
    pic["mf_pred"] = [m[0] for m in pic["mf"]]
    pic["mf_ref"] = [m[1][l] if m[0] >> l & 1 else 0 for m in pic["mf"] for l in range(2)]
    pic["mf_mv"] = [m[2][l][i] if m[0] >> l & 1 else 0 for m in pic["mf"] for l in range(2) for i in range(2)]


def records_of(pic):
    """The kernels' inputs as the picture's fields imply them (bS from the oracle)."""
    bs_v, bs_h = so.boundary_strengths(pic)
    n4 = len(pic["qp"])
    pcm_map = [int(bool(pic["pcm_loop_filter_disabled"] and pic["pcm"][k]) or bool(pic["bypass"][k])) for k in range(n4)]
    slices = []
    for s in pic["slices"]:  # one entry per slice: its dependent segments share the header
        if s["ord"] == len(slices):
            slices.append(dict(beta_offset=2 * s["beta_offset_div2"], tc_offset=2 * s["tc_offset_div2"],
                               across=int(s["across_slices"]), sao_luma=int(s["sao_luma"]), sao_chroma=int(s["sao_chroma"])))
    return dict(name=pic["name"], width=pic["width"], height=pic["height"], log2ctb=pic["log2ctb"], bd_y=pic["bd_y"],
                bd_c=pic["bd_c"], cb_qp_offset=pic["cb_qp_offset"], cr_qp_offset=pic["cr_qp_offset"], bs_v=bs_v, bs_h=bs_h,
                qp=list(pic["qp"]), pcm_map=pcm_map, pcm_nofilter=int(any(pcm_map)), ctb_slice=list(pic["ctb_sord"]),
                ctb_tile=list(pic["ctb_tile"]), slices=slices, sao_params=[dict(p) for p in pic["sao"]],
                deblock=int(any(not s["deblocking_disabled"] for s in pic["slices"])),
                sao=int(any(s["sao_luma"] or s["sao_chroma"] for s in pic["slices"])),
                tiles_block_sao=int(len(set(pic["ctb_tile"])) > 1 and not pic["across_tiles"]), y=pic["y"], uv=pic["uv"])


def oracle_filter(rec, trace=None):
    """The picture after both loop filters, by the oracle (planes in rec["y"], rec["uv"])."""
    prev = so.set_bit_depth(rec["bd_y"])
    try:
        planes = (rec["y"], rec["uv"])
        if rec["deblock"]:
            planes = so.deblock_picture(planes, rec, trace)
        if rec["sao"]:
            planes = so.sao_picture(planes, rec, trace)
        return np.array(planes[0], copy=True), np.array(planes[1], copy=True)
    finally:
        so.set_bit_depth(prev)


_ORACLE = {}


def oracle_cached(rec):
    """oracle_filter once per case name (the CPU and the GPU tests share the results)."""
    if rec["name"] not in _ORACLE:
        _ORACLE[rec["name"]] = oracle_filter(rec)
    return _ORACLE[rec["name"]]


def explain(rec, got, want):
    """None when the planes agree, else the first differing sample."""
    for name, g, w in (("luma", got[0], want[0]), ("chroma", got[1], want[1])):
        if g.shape != w.shape or g.dtype != w.dtype:
            return f"{rec['name']}: {name} plane is {g.dtype}{g.shape}, expected {w.dtype}{w.shape}"
        d = np.argwhere(g != w)
        if len(d):
            r, c = map(int, d[0])
            return f"{rec['name']}: {len(d)} {name} samples differ, first at row {r} column {c}: {int(g[r, c])} != {int(w[r, c])}"
    return None


# ----------------------------------------------------------------------------- coverage
def _luma_tags(lines, bs, qpl, beta_off, tc_off, bd):
    """Which branch of §8.7.2.5.3 / .6 / .7 the edge segment takes (decisions only)."""
    mx = (1 << bd) - 1
    beta = so.BETA_PRIME[so.clip3(0, 51, qpl + beta_off)] << (bd - 8)
    tc = so.TC_PRIME[so.clip3(0, 53, qpl + 2 * (bs - 1) + tc_off)] << (bd - 8)
    P = [[ln[3 - i] for i in range(4)] for ln in lines]
    Q = [[ln[4 + i] for i in range(4)] for ln in lines]
    dp = [abs(P[k][2] - 2 * P[k][1] + P[k][0]) for k in (0, 3)]
    dq = [abs(Q[k][2] - 2 * Q[k][1] + Q[k][0]) for k in (0, 3)]
    if dp[0] + dq[0] + dp[1] + dq[1] >= beta:
        return {"early_out"}

    def dsam(k, dpq):
        return (2 * dpq < beta >> 2 and abs(P[k][3] - P[k][0]) + abs(Q[k][0] - Q[k][3]) < beta >> 3
                and abs(P[k][0] - Q[k][0]) < (5 * tc + 1) >> 1)

    if dsam(0, dp[0] + dq[0]) and dsam(3, dp[1] + dq[1]):
        return {"strong"}
    thr = (beta + (beta >> 1)) >> 3
    tags = set()
    for k in range(4):
        delta = (9 * (Q[k][0] - P[k][0]) - 3 * (Q[k][1] - P[k][1]) + 8) >> 4
        if abs(delta) >= 10 * tc:
            tags.add("skip_10tc")
            continue
        tags |= {"normal", "dEp1" if sum(dp) < thr else "dEp0", "dEq1" if sum(dq) < thr else "dEq0"}
        delta = so.clip3(-tc, tc, delta)
        for v in (P[k][0] + delta, Q[k][0] - delta):
            if v < 0:
                tags.add("clip_0")
            if v > mx:
                tags.add("clip_max")
    return tags


DEBLOCK_TAGS = {"bs0", "bs1", "bs2", "early_out", "strong", "normal", "dEp0", "dEp1", "dEq0", "dEq1", "skip_10tc",
                "clip_0", "clip_max", "chroma", "chroma_skip_bs1", "chroma_skip_grid", "nfp_only", "nfq_only",
                "slice_offsets_meet", "qp_differs"}
SAO_TAGS = set()
for _c in range(3):
    SAO_TAGS |= {(_c, "band", k) for k in range(1, 5)} | {(_c, "band_wrap")}
    SAO_TAGS |= {(_c, "eo", cl, e) for cl in range(4) for e in range(5)}
    SAO_TAGS |= {(_c, "refused", "border", s) for s in ("left", "right", "top", "bottom")}
    SAO_TAGS |= {(_c, r, w) for r in ("refused", "allowed") for w in ("tile", "earlier", "later")}
    SAO_TAGS |= {(_c, "clip_0"), (_c, "clip_max"), (_c, "exempt"), (_c, "exempt_nb"), (_c, "type0_beside")}
SAO_TAGS |= {"sao_luma_only", "sao_chroma_only"}


def coverage(rec):
    """Everything the record reaches, from the oracle's trace."""
    trace = []
    oracle_filter(rec, trace)
    bd, mx = rec["bd_y"], (1 << rec["bd_y"]) - 1
    w4 = rec["width"] // 4
    tags = set()
    if rec["deblock"]:
        for d, m in ((0, rec["bs_v"]), (1, rec["bs_h"])):
            for b, v in enumerate(m):
                pos = 4 * (b % w4 if d == 0 else b // w4)
                if pos and pos % 8 == 0:
                    tags.add(f"bs{v}")
    for t in trace:
        if t[0] == "luma":
            _, d, x, y, bs, lines, out, qpp, qpq, nfp, nfq, beta_off, tc_off = t
            lt = _luma_tags(lines, bs, (qpp + qpq + 1) >> 1, beta_off, tc_off, bd)
            tags |= lt
            if lt & {"strong", "normal"}:
                if nfp and not nfq:
                    tags.add("nfp_only")
                if nfq and not nfp:
                    tags.add("nfq_only")
            if qpp != qpq:
                tags.add("qp_differs")
            xp, yp = (x - 1, y) if d == 0 else (x, y - 1)
            sp = rec["slices"][rec["ctb_slice"][so._ctb_of(rec, xp, yp)]]
            sq = rec["slices"][rec["ctb_slice"][so._ctb_of(rec, x, y)]]
            if (sp["beta_offset"], sp["tc_offset"]) != (sq["beta_offset"], sq["tc_offset"]):
                tags.add("slice_offsets_meet")
        elif t[0] == "chroma":
            tags.add("chroma")
        elif t[0] == "chroma_skip":
            tags.add("chroma_skip_bs1" if t[4] == 1 else "chroma_skip_grid")
        elif t[0] == "exempt":
            tags.add((t[1], "exempt"))
        elif t[0] == "exempt_nb":
            tags.add((t[1], "exempt_nb"))
        elif t[0] == "allowed":
            tags.add((t[1], "allowed", t[2]))
        elif t[0] == "refused":
            _, c, why, dx, dy = t
            if why == "border":
                if dy == 0:
                    tags.add((c, "refused", "border", "left" if dx < 0 else "right"))
                elif dx == 0:
                    tags.add((c, "refused", "border", "top" if dy < 0 else "bottom"))
            else:
                tags.add((c, "refused", why))
        elif t[0] == "sao":
            _, c, x, y, typ, band, eo, nb, v, off = t
            cur = nb[1][1]
            if typ == 1:
                k = ((cur >> (bd - 5)) - band) & 31
                if k < 4:
                    tags.add((c, "band", k + 1))
                    if band + k > 31:
                        tags.add((c, "band_wrap"))
                    raw = cur + off[k]
                else:
                    raw = cur
            else:
                e = 2 + sum(so.sign(cur - nb[1 + dy][1 + dx]) for dx, dy in so.SAO_EO_OFFSETS[eo])
                e = (0 if e == 2 else e + 1) if e <= 2 else e
                tags.add((c, "eo", eo, e))
                raw = cur + ([0] + list(off))[e]
            if raw < 0:
                tags.add((c, "clip_0"))
            if raw > mx:
                tags.add((c, "clip_max"))
    if rec["sao"]:
        ctb = 1 << rec["log2ctb"]
        wctb = (rec["width"] + ctb - 1) // ctb
        for k, p in enumerate(rec["sao_params"]):
            if k % wctb == 0:
                continue
            q = rec["sao_params"][k - 1]
            for c in range(3):
                on = all(rec["slices"][rec["ctb_slice"][j]]["sao_luma" if c == 0 else "sao_chroma"] for j in (k, k - 1))
                if on and bool(p["type"][c]) != bool(q["type"][c]):
                    tags.add((c, "type0_beside"))
        for s in rec["slices"]:
            if s["sao_luma"] and not s["sao_chroma"]:
                tags.add("sao_luma_only")
            if s["sao_chroma"] and not s["sao_luma"]:
                tags.add("sao_chroma_only")
    return tags


# ----------------------------------------------------------------------------- the cases
def _sl(ord_, **kw):
    return default_slice(ord=ord_, **kw)


_REFS_B = ([11, 10, 12], [10, 12])  # index 0 of list 0 names another picture than in default_slice


def shape_cases():
    """One picture per shape of the issue; together they reach every deblocking and SAO branch."""
    dbk = tuple(sorted(DEBLOCK_TAGS - {"slice_offsets_meet"}))

    def rim(luma, chroma):
        return [(c, "refused", "border", s) for c in range(3) for s in (chroma if c else luma)]

    return [
        make_pic(1, 16, 16, 4, sao_eo=(0, 1), name="16x16_rim_eo_0_1", reach=rim(("left", "right"), ("top", "bottom"))),
        make_pic(9, 16, 16, 4, sao_eo=(1, 0), name="16x16_rim_eo_1_0", reach=rim(("top", "bottom"), ("left", "right"))),
        make_pic(30, 24, 16, 4, reach=["bs2", "chroma"]),
        make_pic(3, 72, 40, 6, reach=["bs0", "bs1", "bs2", "strong", "normal", "early_out"]),
        make_pic(4, 72, 40, 5, cqp=(3, -4), reach=["bs0", "bs1", "bs2", "chroma", "qp_differs"]),
        make_pic(5, 40, 72, 4, cqp=(-2, 5), reach=["bs0", "bs1", "bs2", "chroma_skip_grid", "chroma_skip_bs1"]),
        make_pic(6, 136, 72, 5, reach=dbk),
        make_pic(7, 24, 16, 4, bd=10, reach=["bs2", "chroma"]),
        make_pic(8, 72, 40, 6, bd=10, reach=["bs0", "bs1", "bs2", "strong", "normal", "nfp_only", "nfq_only"]),
    ]


def layout_cases():
    """72x40 at CTB 16 (5 x 3 CTBs): slices split mid-row, tiles, and both."""
    two_a = [_sl(0, beta_offset_div2=-2, tc_offset_div2=3, across_slices=1, sao_chroma=0),
             _sl(1, beta_offset_div2=4, tc_offset_div2=-3, across_slices=0, ref_lists=_REFS_B)]
    two_b = [_sl(0, beta_offset_div2=5, tc_offset_div2=0, across_slices=0, sao_luma=0),
             _sl(1, beta_offset_div2=-4, tc_offset_div2=2, across_slices=1, ref_lists=_REFS_B)]
    three = [_sl(0, across_slices=1), _sl(1, across_slices=0, deblocking_disabled=1, ref_lists=_REFS_B),
             _sl(1, across_slices=0, deblocking_disabled=1, ref_lists=_REFS_B), _sl(2, across_slices=1, tc_offset_div2=6)]
    refused = [(c, "refused", w) for c in range(3) for w in ("earlier", "later")]
    allowed = [(c, "allowed", w) for c in range(3) for w in ("earlier", "later")]
    # (two_a switches chroma SAO off in its first slice, two_b luma SAO: those samples meet no later slice)
    refused_a = [t for t in refused if t[0] == 0 or t[2] == "earlier"]
    allowed_b = [t for t in allowed if t[0] != 0 or t[2] == "earlier"]
    return [
        make_pic(11, 72, 40, 4, slices=two_a, starts=(0, 7), name="slices_mid_row_10", reach=refused_a + ["sao_luma_only"]),
        make_pic(12, 72, 40, 4, slices=two_b, starts=(0, 7), name="slices_mid_row_01",
                 reach=allowed_b + ["slice_offsets_meet", "sao_chroma_only"]),
        make_pic(40, 72, 40, 4, slices=[_sl(0, across_slices=0, tc_offset_div2=-1), _sl(1, across_slices=0, beta_offset_div2=1,
                                                                                        ref_lists=_REFS_B)],
                 starts=(0, 7), name="slices_mid_row_00", reach=refused),
        make_pic(40, 72, 40, 4, slices=[_sl(0, across_slices=1, tc_offset_div2=-1), _sl(1, across_slices=1, beta_offset_div2=1,
                                                                                        ref_lists=_REFS_B)],
                 starts=(0, 7), name="slices_mid_row_11", reach=allowed + ["slice_offsets_meet"]),
        make_pic(13, 72, 40, 4, slices=three, starts=(0, 4, 6, 11), name="slices_dependent_segment", reach=refused + allowed),
        make_pic(14, 72, 40, 4, tiles=dict(cols=2, rows=2), across_tiles=0, name="tiles_2x2_cut",
                 reach=[(c, "refused", "tile") for c in range(3)]),
        make_pic(15, 72, 40, 4, tiles=dict(cols=2, rows=2), across_tiles=1, name="tiles_2x2_across",
                 reach=[(c, "allowed", "tile") for c in range(3)]),
        make_pic(16, 72, 40, 4, tiles=dict(cols=3, rows=1, uniform=False, col_width=(1, 3)), across_tiles=0,
                 name="tiles_explicit_columns", reach=[(c, "refused", "tile") for c in range(3)]),
        make_pic(30, 72, 40, 4, tiles=dict(cols=2, rows=1), across_tiles=0, slices=two_b, starts=(0, 9),
                 name="tiles_and_slices", reach=[(c, "refused", "tile") for c in range(3)] + [(c, "allowed", "earlier") for c in range(3)]),
        make_pic(30, 72, 40, 4, tiles=dict(cols=2, rows=1), across_tiles=1, slices=two_a, starts=(0, 4),
                 name="tiles_and_slices_10", reach=[(c, "allowed", "tile") for c in range(3)] + refused_a),
    ]


def all_pictures():
    return shape_cases() + layout_cases()


def batch_cases():
    """(name, records) of the two batches: mixed sizes and depths in one launch."""
    a = records_of(make_pic(21, 136, 72, 5, name="batch_136x72"))
    b = records_of(make_pic(22, 24, 16, 4, bd=10, name="batch_24x16_10bit"))
    c = records_of(make_pic(23, 72, 40, 5, slices=[_sl(0, deblocking_disabled=1)], name="batch_72x40_sao_only"))
    d = records_of(make_pic(24, 16, 16, 4, slices=[_sl(0, deblocking_disabled=1, sao_luma=0, sao_chroma=0)],
                            name="batch_16x16_unfiltered"))
    assert (c["deblock"], c["sao"], d["deblock"], d["sao"]) == (0, 1, 0, 0)
    e = records_of(make_pic(25, 72, 40, 4, slices=[_sl(0, sao_luma=0, sao_chroma=0)], name="batch_72x40_no_sao"))
    f = records_of(make_pic(26, 40, 72, 4, bd=10, slices=[_sl(0, sao_luma=0, sao_chroma=0)], name="batch_40x72_10bit_no_sao"))
    assert not (e["sao"] or f["sao"] or d["sao"])
    return [("mixed_four", [a, b, c, d]), ("no_sao", [e, f, d])]


# ----------------------------------------------------------------------------- bS table (§8.7.2.4)
def _two_block(name, want, p, q, edge="tu", pos=8, horizontal=False, slices=None, split=False, tiles=1, across_tiles=1):
    """A 32x16 picture of two CTBs (16x32 when `horizontal`: the edge under test is horizontal):
    everything before `pos` is the p side, the rest the q side; only the line at `pos` carries edge
    flags. split: the second CTB is another slice segment; tiles 2: another tile."""
    w, h = (16, 32) if horizontal else (32, 16)
    w4, h4 = w // 4, h // 4
    n4 = w4 * h4
    slices = slices or [default_slice()]
    lay = dict(cols=1, rows=tiles) if horizontal else dict(cols=tiles, rows=1)
    ctb_tile, _ = tile_layout(w // 16, h // 16, lay["cols"], lay["rows"])
    pic = dict(name=name, want=want, pos=pos, horizontal=horizontal, width=w, height=h, log2ctb=4, bd_y=8, bd_c=8,
               cb_qp_offset=0, cr_qp_offset=0, pcm_loop_filter_disabled=0, transquant_bypass=0, tile_cols=lay["cols"],
               tile_rows=lay["rows"], uniform_spacing=1, col_width=[], row_height=[], across_tiles=across_tiles,
               slices=slices, ctb_slice=[0, 1 if split else 0], ctb_tile=ctb_tile)
    pic["ctb_sord"] = [slices[k]["ord"] for k in pic["ctb_slice"]]
    side = dict(intra=0, cbf=0, pred=1, ref=(0, 0), mv=((0, 0), (0, 0)))
    keys = ("intra", "cbf", "tu_v", "tu_h", "pu_v", "pu_h")
    for k in keys:
        pic[k] = [0] * n4
    pic["mf"] = [None] * n4
    for b in range(n4):
        at = 4 * (b // w4 if horizontal else b % w4)
        s = dict(side, **(q if at >= pos else p))
        pic["intra"][b], pic["cbf"][b] = s["intra"], s["cbf"]
        pic["mf"][b] = (0, (0, 0), ((0, 0), (0, 0))) if s["intra"] else (s["pred"], tuple(s["ref"]), tuple(map(tuple, s["mv"])))
        if at == pos:
            pic["tu_h" if horizontal else "tu_v"][b] = int(edge in ("tu", "both"))
            pic["pu_h" if horizontal else "pu_v"][b] = int(edge in ("pu", "both"))
    pic.update(qp=[30] * n4, pcm=[0] * n4, bypass=[0] * n4)
    pic["y"], pic["uv"] = make_planes(random.Random(len(name)), w, h, 8)
    pic["sao"] = [dict(type=[0, 0, 0], band=[0, 0, 0], eo=[0, 0, 0], off=[[0] * 4 for _ in range(3)]) for _ in range(2)]
    _binding_fields(pic)
    return pic


def bs_table():
    """Two-block pictures, one clause of §8.7.2.4 each; `want` is the bS of the edge under test,
    written here from the clause (the oracle must agree)."""
    T = _two_block
    bi = dict(pred=3, ref=(0, 0))  # default lists: L0[0] = 10, L1[0] = 11
    two = [_sl(0), _sl(1, ref_lists=_REFS_B)]
    return [
        T("intra_p", 2, dict(intra=1), {}),
        T("intra_q", 2, {}, dict(intra=1)),
        T("intra_on_pu_edge", 2, dict(intra=1), {}, edge="pu"),
        T("cbf_tu_edge", 1, dict(cbf=1), {}),
        T("cbf_q_tu_edge", 1, {}, dict(cbf=1)),
        T("cbf_pu_only_edge", 0, dict(cbf=1), dict(cbf=1), edge="pu"),
        T("mv_count_differs", 1, dict(pred=1), dict(pred=3), edge="pu"),
        T("different_pictures", 1, dict(ref=(0, 0)), dict(ref=(1, 0))),                 # 10 against 11
        T("same_picture_two_indices", 0, dict(ref=(0, 0)), dict(ref=(2, 0))),           # L0[0] = L0[2] = 10
        T("same_picture_two_lists", 0, dict(pred=1, ref=(1, 0)), dict(pred=2, ref=(0, 0))),  # L0[1] = L1[0] = 11
        T("same_index_two_slices", 1, dict(ref=(0, 0)), dict(ref=(0, 0)), pos=16, slices=two, split=True),  # 10 / 11
        T("other_index_same_picture_two_slices", 0, dict(ref=(0, 0)), dict(ref=(1, 0)), pos=16, slices=two, split=True),
        T("mv_dx_3", 0, {}, dict(mv=((3, 0), (0, 0)))),
        T("mv_dx_4", 1, {}, dict(mv=((4, 0), (0, 0)))),
        T("mv_dx_minus_4", 1, {}, dict(mv=((-4, 0), (0, 0)))),
        T("mv_dy_3", 0, {}, dict(mv=((0, 3), (0, 0)))),
        T("mv_dy_4", 1, {}, dict(mv=((0, 4), (0, 0)))),
        T("bi_straight_match", 0, dict(bi, mv=((0, 0), (8, 8))), dict(bi, mv=((3, 0), (8, 5)))),
        T("bi_straight_far", 1, dict(bi, mv=((0, 0), (8, 8))), dict(bi, mv=((3, 0), (8, 4)))),
        # p: L0[0] = 10, L1[0] = 11; q lies in the second slice, where L0[0] = 11 and L1[0] = 10
        T("bi_crossed_match", 0, dict(bi, mv=((0, 0), (8, 8))), dict(bi, mv=((8, 8), (0, 0))), pos=16, slices=two, split=True),
        T("bi_crossed_far", 1, dict(bi, mv=((0, 0), (8, 8))), dict(bi, mv=((8, 4), (0, 0))), pos=16, slices=two, split=True),
        T("bi_crossed_not_straight", 1, dict(bi, mv=((0, 0), (8, 8))), dict(bi, mv=((0, 0), (8, 8))), pos=16, slices=two,
          split=True),  # q's vectors point at the other pictures: the same numbers do not match
        # both vectors of both sides to picture 11: L0[1] and L1[0]
        T("bi_same_picture_straight_only", 0, dict(pred=3, ref=(1, 0), mv=((0, 0), (8, 8))),
          dict(pred=3, ref=(1, 0), mv=((0, 0), (8, 8)))),
        T("bi_same_picture_crossed_only", 0, dict(pred=3, ref=(1, 0), mv=((0, 0), (8, 8))),
          dict(pred=3, ref=(1, 0), mv=((8, 8), (0, 0)))),
        T("bi_same_picture_both_fail", 1, dict(pred=3, ref=(1, 0), mv=((0, 0), (8, 8))),
          dict(pred=3, ref=(1, 0), mv=((0, 4), (8, 4)))),
        T("bi_same_picture_half_of_each_pairing", 1, dict(pred=3, ref=(1, 0), mv=((0, 0), (8, 8))),
          dict(pred=3, ref=(1, 0), mv=((0, 4), (0, 0)))),  # straight fails at (0,0)-(0,4), crossed at (8,8)-(0,4)
        T("edge_at_4", 0, dict(intra=1), dict(intra=1), pos=4),
        T("edge_at_12", 0, dict(intra=1), dict(intra=1), pos=12),
        T("edge_at_12_horizontal", 0, dict(intra=1), dict(intra=1), pos=12, horizontal=True),
        T("horizontal_intra", 2, dict(intra=1), {}, horizontal=True),
        T("slice_boundary_q_flag_1", 2, dict(intra=1), {}, pos=16, split=True,
          slices=[_sl(0, across_slices=0), _sl(1, across_slices=1)]),
        T("slice_boundary_q_flag_0", 0, dict(intra=1), {}, pos=16, split=True,
          slices=[_sl(0, across_slices=1), _sl(1, across_slices=0)]),
        T("dependent_segment_is_no_slice_boundary", 2, dict(intra=1), {}, pos=16, split=True,
          slices=[_sl(0, across_slices=0), _sl(0, across_slices=0)]),
        T("tile_boundary_flag_1", 2, dict(intra=1), {}, pos=16, tiles=2, across_tiles=1),
        T("tile_boundary_flag_0", 0, dict(intra=1), {}, pos=16, tiles=2, across_tiles=0),
        T("q_slice_disabled_under_enabled", 0, dict(intra=1), {}, pos=16, split=True, horizontal=True,
          slices=[_sl(0), _sl(1, deblocking_disabled=1)]),
        T("q_slice_enabled_under_disabled", 2, dict(intra=1), {}, pos=16, split=True, horizontal=True,
          slices=[_sl(0, deblocking_disabled=1), _sl(1)]),
    ]
