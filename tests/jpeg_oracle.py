"""Independent oracles of the JPEG encoder (csrc/vep/jpeg.h, jpeg.cpp, gpu_jpeg.hip) and the rules
that compare an encoder with them. numpy float64 and Python ints only: the module takes no
constant and no function from the package or the extension, so a slip in jpeg.h, which the CPU
encoder and the kernels share line by line, cannot hide in a shared helper. A helper module like
letterbox_oracle.py; test_jpeg_oracle.py (CPU) and test_gpu_jpeg_oracle.py (MI355X) use it.

Four parts:

a) ``read_stream``: a strict baseline (SOF0) stream reader in pure Python. Everything comes from
   the stream: quantisation tables from DQT, the Huffman decoding tables from the DHT segments,
   the interval length from DRI, the zigzag order from the walk of the diagonals. It returns the
   quantised coefficients of every block in natural order and asserts what a strict decoder would
   (stuffing, interval lengths, padding, RSTm cycle, EOI).
b) ``luma_plane``: dequantise and reconstruct the luma plane with a float64 IDCT. Its only use is
   to validate the reader against libjpeg.
c) ``format_coefficients``: the arithmetic of the format as the header comment of jpeg.h and
   docs/JPEG.md state it, restated in numpy int64 from those words: edge replication, the three
   16.16 colour formulas, ``(a + b + c + d + 2) >> 2``, the level shift, the two DCT passes with
   their shifts, round-half-away quantisation, the IJG table scaling. It pins the implementation
   to the documented format with zero tolerance (the *exact rule*).
d) ``float_coefficients``: the mathematics. JFIF colour in float64, the orthonormal float64 DCT-II
   built from cos, applied to the 8-bit samples (JPEG defines the DCT on 8-bit samples), divided by
   the quantiser. It pins the format to the mathematics (the *float rule* and the *colour rule*).

The 8-bit samples of (d). A sample is floor(f + 0.5) of its float64 JFIF value f wherever the
colour rule decides it. About 1 % of all colours are undecidable (below); there (d) takes the value
of the documented 16.16 formula after asserting that it is one of the two neighbours. A chroma
sample is then the float64 mean of the four 8-bit samples rounded half up, which is exact.

Error bound of the format's integer transform (``bound``), from its stated precision alone. The
matrix entries are the orthonormal ones rounded to 13 fraction bits: each carries an error of at
most 2^-14. The row pass keeps 3 fraction bits: its rounding is at most 2^-4. The column pass and
the 16 fraction bits before the quantiser add nothing. With real-unit (level-shifted) samples p,
C the orthonormal matrix and t = the float64 row pass,

    eps_t[y]    = 2^-14 * sum_x |p[y][x]| + 2^-4
    eps_d[v][u] = sum_y (|C[v][y]| + 2^-14) * eps_t[y] + 2^-14 * sum_y |t[y][u]|

The first sum carries the row pass's error through the (rounded) column matrix, the second is the
column matrix's own rounding acting on the row values.

Clamps. The format clamps AC to +-1023 and the DC difference to +-2047. With 8-bit input neither
can be reached: the largest AC magnitude of a sign-of-basis block at Q = 1 is 1020 and the largest
DC difference 2040. The oracles do not model the clamps; they assert that nothing they produce
needs one.
"""
from collections import namedtuple

import numpy as np

# ------------------------------------------------------------------------------------ (a) reader

Stream = namedtuple("Stream", "w h sampling tq qt dri coefs markers rst interval_mcus mcus_x mcus_y")


def zigzag_order():
    """zigzag index -> natural position (row * 8 + column), from the walk of the anti-diagonals:
    diagonal s = row + column, upwards (row falling) for even s, downwards for odd s."""
    out = []
    for s in range(15):
        rows = range(min(s, 7), max(0, s - 7) - 1, -1) if s % 2 == 0 else range(max(0, s - 7), min(s, 7) + 1)
        out += [r * 8 + (s - r) for r in rows]
    assert sorted(out) == list(range(64))
    return out


ZZ = zigzag_order()


def _decoding_table(bits, vals):
    """16-bit lookup table of one DHT specification (Annex C code assignment): entry = length << 8
    | symbol for every 16-bit window that starts with a code, -1 where no code matches."""
    lut = [-1] * 65536
    code, k = 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            assert code < (1 << length), "DHT: more codes than the length allows"
            lo = code << (16 - length)
            lut[lo:lo + (1 << (16 - length))] = [length << 8 | vals[k]] * (1 << (16 - length))
            code += 1
            k += 1
        code <<= 1
    assert k == len(vals)
    return lut


class _Bits:
    """MSB-first reader over one interval's unstuffed bytes."""

    def __init__(self, data):
        self.buf = bytes(data) + b"\0\0\0"
        self.total = 8 * len(data)
        self.pos = 0

    def peek16(self):
        i = self.pos >> 3
        b = self.buf
        return ((b[i] << 16 | b[i + 1] << 8 | b[i + 2]) >> (8 - (self.pos & 7))) & 0xFFFF

    def skip(self, n):
        self.pos += n
        assert self.pos <= self.total, "entropy data ends inside a symbol"

    def symbol(self, lut):
        e = lut[self.peek16()]
        assert e >= 0, f"bits at {self.pos} are no code of the table (every symbol must have a code)"
        self.skip(e >> 8)
        return e & 0xFF

    def value(self, s):
        """s extra bits as the signed value of category s (F.2.2.1 EXTEND)."""
        if s == 0:
            return 0
        v = self.peek16() >> (16 - s)
        self.skip(s)
        return v if v >= (1 << (s - 1)) else v - (1 << s) + 1


def _be16(b, i):
    return b[i] << 8 | b[i + 1]


def read_stream(data):
    """Parse and decode a baseline JPEG stream. Returns a ``Stream``:
    w, h; sampling [(H, V)] per component; tq [table id] per component; qt {id: int64 [64] in
    natural order}; dri (0: none); coefs int64 [mcus, blocks per MCU, 64] in natural order, the
    MCU's blocks in scan order; markers [second byte] up to SOS in order; rst [m of every RSTm];
    interval_mcus [MCUs decoded per interval]; mcus_x, mcus_y."""
    data = bytes(data)
    assert data[:2] == b"\xff\xd8", "SOI expected"
    markers, i = [0xD8], 2
    qt, huff, comps, dri, w, h, scan = {}, {}, None, 0, None, None, None
    while scan is None:
        assert data[i] == 0xFF, f"marker expected at byte {i}"
        m = data[i + 1]
        n = _be16(data, i + 2)
        seg = data[i + 4:i + 2 + n]
        assert len(seg) == n - 2, "segment runs past the end"
        markers.append(m)
        i += 2 + n
        if 0xE0 <= m <= 0xEF or m == 0xFE:  # APPn, COM
            if m == 0xE0 and len(markers) == 2:
                assert seg[:5] == b"JFIF\0", "APP0 is not JFIF"
        elif m == 0xDB:
            k = 0
            while k < len(seg):
                pq, tq = seg[k] >> 4, seg[k] & 15
                assert pq == 0, "baseline: 8-bit quantisation tables"
                t = np.zeros(64, dtype=np.int64)
                for z in range(64):
                    t[ZZ[z]] = seg[k + 1 + z]
                assert t.min() >= 1
                qt[tq] = t
                k += 65
            assert k == len(seg)
        elif m == 0xC0:
            assert seg[0] == 8, "8-bit samples"
            h, w = _be16(seg, 1), _be16(seg, 3)
            assert w >= 1 and h >= 1
            assert len(seg) == 6 + 3 * seg[5]
            comps = [(seg[6 + 3 * c], seg[7 + 3 * c] >> 4, seg[7 + 3 * c] & 15, seg[8 + 3 * c]) for c in range(seg[5])]
        elif m == 0xC4:
            k = 0
            while k < len(seg):
                tc_th = seg[k]
                assert tc_th >> 4 in (0, 1) and tc_th & 15 in (0, 1), "baseline: two tables per class"
                bits = list(seg[k + 1:k + 17])
                nv = sum(bits)
                vals = list(seg[k + 17:k + 17 + nv])
                assert len(vals) == nv
                huff[tc_th] = _decoding_table(bits, vals)
                k += 17 + nv
            assert k == len(seg)
        elif m == 0xDD:
            assert n == 4
            dri = _be16(seg, 0)
        elif m == 0xDA:
            assert comps is not None, "SOS before SOF0"
            assert seg[0] == len(comps), "one interleaved scan of all components"
            scan = []
            for c in range(seg[0]):
                assert seg[1 + 2 * c] == comps[c][0], "scan components in frame order"
                scan.append((seg[2 + 2 * c] >> 4, seg[2 + 2 * c] & 15))
            assert tuple(seg[1 + 2 * seg[0]:]) == (0, 63, 0), "baseline scan: Ss 0, Se 63, Ah Al 0"
        else:
            raise AssertionError(f"marker 0x{m:02x} is not part of a baseline stream this reader accepts")

    # entropy data: split at the markers, take out the stuffing
    intervals, rst, cur = [], [], bytearray()
    while True:
        j = data.find(b"\xff", i)
        assert j >= 0 and j + 1 < len(data), "entropy data without EOI"
        cur += data[i:j]
        m = data[j + 1]
        if m == 0x00:
            cur.append(0xFF)
        elif 0xD0 <= m <= 0xD7:
            rst.append(m - 0xD0)
            intervals.append(bytes(cur))
            cur = bytearray()
        else:
            assert m == 0xD9, f"0xFF in entropy data is followed by 0x{m:02x}: not 0x00, RSTm or EOI"
            assert j + 2 == len(data), "EOI does not end the stream"
            intervals.append(bytes(cur))
            break
        i = j + 2
    assert rst == [k % 8 for k in range(len(rst))], f"RSTm does not cycle 0..7: {rst[:12]}"

    hmax, vmax = max(c[1] for c in comps), max(c[2] for c in comps)
    mcus_x, mcus_y = -(-w // (8 * hmax)), -(-h // (8 * vmax))
    mcus = mcus_x * mcus_y
    per = dri if dri else mcus
    assert len(intervals) == -(-mcus // per), f"{len(intervals)} intervals for {mcus} MCUs at DRI {dri}"
    layout = []  # (component, dc table, ac table) per block of an MCU
    for c, (_, hh, vv, tq) in enumerate(comps):
        assert tq in qt, "component names a missing quantisation table"
        td, ta = scan[c]
        layout += [(c, huff[td], huff[0x10 | ta])] * (hh * vv)
    coefs = np.zeros((mcus, len(layout), 64), dtype=np.int64)
    interval_mcus, m0 = [], 0
    for seg in intervals:
        cnt = min(per, mcus - m0)  # every interval holds exactly DRI MCUs, the last the remainder
        br = _Bits(seg)
        pred = [0] * len(comps)  # DC prediction restarts at every interval
        for mcu in range(m0, m0 + cnt):
            for b, (c, dc, ac) in enumerate(layout):
                s = br.symbol(dc)
                assert s <= 11, "DC category above 11"
                pred[c] += br.value(s)
                row = coefs[mcu, b]
                row[0] = pred[c]
                k = 1
                while k < 64:
                    rs = br.symbol(ac)
                    r, s = rs >> 4, rs & 15
                    if s == 0:
                        if r == 0:
                            break  # EOB
                        assert r == 15, "baseline has no EOBn"
                        k += 16
                        assert k < 64, "ZRL runs past the block"
                        continue
                    assert s <= 10, "AC category above 10"
                    k += r
                    assert k < 64, "run past the block"
                    row[ZZ[k]] = br.value(s)
                    k += 1
        left = br.total - br.pos
        assert left < 8, f"{left} bits remain after the interval's last MCU"
        if left:
            assert (br.peek16() >> (16 - left)) == (1 << left) - 1, "padding bits are not all 1"
        interval_mcus.append(cnt)
        m0 += cnt
    assert m0 == mcus
    return Stream(w, h, [(c[1], c[2]) for c in comps], [c[3] for c in comps], qt, dri, coefs, markers, rst,
                  interval_mcus, mcus_x, mcus_y)


# ------------------------------------------------------------------------- (b) luma reconstruction

def dct_matrix():
    """Orthonormal DCT-II: C[u][x] = c(u) / 2 * cos((2x + 1) u pi / 16), c(0) = 1 / sqrt(2)."""
    u = np.arange(8, dtype=np.float64).reshape(8, 1)
    x = np.arange(8, dtype=np.float64).reshape(1, 8)
    C = 0.5 * np.cos((2.0 * x + 1.0) * u * np.pi / 16.0)
    C[0] *= 1.0 / np.sqrt(2.0)
    return C


C = dct_matrix()


def luma_plane(st):
    """uint8 [h, w] luma of a read stream: dequantise, float64 IDCT, + 128, round, clamp."""
    H, V = st.sampling[0]
    q = st.qt[st.tq[0]].astype(np.float64)
    F = (st.coefs[:, :H * V] * q).reshape(st.mcus_y, st.mcus_x, V, H, 8, 8)
    px = np.einsum("vy,...vu,ux->...yx", C, F, C)  # sum_v sum_u C[v][y] F[v][u] C[u][x]
    plane = px.transpose(0, 2, 4, 1, 3, 5).reshape(st.mcus_y * V * 8, st.mcus_x * H * 8)
    return np.clip(np.floor(plane + 128.0 + 0.5), 0, 255).astype(np.uint8)[:st.h, :st.w]


# ------------------------------------------------------------------- (c) the documented arithmetic

RESTART_INTERVAL = 3  # MCUs, as docs/JPEG.md states it; the tests check the stream's DRI against it

# ITU-T T.81 Annex K, tables K.1 (luminance) and K.2 (chrominance), natural order
K1 = np.array([16, 11, 10, 16, 24, 40, 51, 61,
               12, 12, 14, 19, 26, 58, 60, 55,
               14, 13, 16, 24, 40, 57, 69, 56,
               14, 17, 22, 29, 51, 87, 80, 62,
               18, 22, 37, 56, 68, 109, 103, 77,
               24, 35, 55, 64, 81, 104, 113, 92,
               49, 64, 78, 87, 103, 121, 120, 101,
               72, 92, 95, 98, 112, 100, 103, 99], dtype=np.int64)
K2 = np.full(64, 99, dtype=np.int64)
K2.reshape(8, 8)[:4, :4] = [[17, 18, 24, 47], [18, 21, 26, 66], [24, 26, 56, 99], [47, 66, 99, 99]]


def ijg_tables(quality):
    """(luma, chroma) int64 [64] in natural order: scale = 5000 / q below 50, 200 - 2 q otherwise;
    entry (t * scale + 50) / 100 clamped to 1..255."""
    assert 1 <= quality <= 100
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    return tuple(np.clip((t * scale + 50) // 100, 1, 255) for t in (K1, K2))


def replicate(bgr):
    """[h, w, 3] -> int64 [16 * mcus_y, 16 * mcus_x, 3]: the last column / row repeated."""
    bgr = np.asarray(bgr)
    assert bgr.ndim == 3 and bgr.shape[2] == 3 and bgr.dtype == np.uint8
    h, w = bgr.shape[:2]
    ys = np.minimum(np.arange(-(-h // 16) * 16), h - 1)
    xs = np.minimum(np.arange(-(-w // 16) * 16), w - 1)
    return bgr[ys][:, xs].astype(np.int64)


def format_colour(b, g, r):
    """The three 16.16 formulas; int64 arrays in, (Y, Cb, Cr) out. >> is arithmetic."""
    b, g, r = (np.asarray(v, dtype=np.int64) for v in (b, g, r))
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    return y, cb, cr


def _mcu_blocks(y, cb, cr):
    """Sample planes (luma [H, W], chroma [H/2, W/2]; H, W multiples of 16) -> [mcus, 6, 8, 8]
    in the MCU's block order Y00 Y01 Y10 Y11 Cb Cr, MCUs in raster order."""
    my, mx = y.shape[0] // 16, y.shape[1] // 16
    yb = y.reshape(my, 2, 8, mx, 2, 8).transpose(0, 3, 1, 4, 2, 5).reshape(my * mx, 4, 8, 8)
    cbb = cb.reshape(my, 8, mx, 8).transpose(0, 2, 1, 3).reshape(my * mx, 1, 8, 8)
    crb = cr.reshape(my, 8, mx, 8).transpose(0, 2, 1, 3).reshape(my * mx, 1, 8, 8)
    return np.concatenate([yb, cbb, crb], axis=1)


def _quant_blocks(quality):
    ql, qc = ijg_tables(quality)
    return np.stack([ql] * 4 + [qc] * 2).reshape(6, 8, 8)


def _assert_no_clamp(coefs, interval):
    """coefs [mcus, 6, 64]: no AC beyond +-1023, no DC difference beyond +-2047 (prediction per
    component, restarting every `interval` MCUs)."""
    if coefs.size == 0:
        return
    assert np.abs(coefs[:, :, 1:]).max() <= 1023, "an AC coefficient needs the clamp"
    pred = np.zeros(3, dtype=np.int64)
    comp = [0, 0, 0, 0, 1, 2]
    for m in range(coefs.shape[0]):
        if m % interval == 0:
            pred[:] = 0
        for b in range(6):
            assert abs(int(coefs[m, b, 0]) - int(pred[comp[b]])) <= 2047, "a DC difference needs the clamp"
            pred[comp[b]] = coefs[m, b, 0]


def format_samples(bgr):
    """Level-shifted sample blocks int64 [mcus, 6, 8, 8] of the documented arithmetic."""
    p = replicate(bgr)
    y, cb, cr = format_colour(p[..., 0], p[..., 1], p[..., 2])
    for v in (y, cb, cr):
        assert v.min() >= 0 and v.max() <= 255
    mean = lambda c: (c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2] + 2) >> 2
    return _mcu_blocks(y, mean(cb), mean(cr)) - 128


def format_dct(p):
    """The two integer passes on level-shifted sample blocks int64 [..., y, x] -> d [..., v, u]
    with 16 fraction bits."""
    K = np.rint(2.0 ** 13 * C).astype(np.int64)  # "the orthonormal DCT-II matrix scaled by 2^13"
    t = (np.einsum("ux,...yx->...yu", K, p) + 512) >> 10  # 3 fraction bits
    d = np.einsum("vy,...yu->...vu", K, t)
    if d.size:
        assert np.abs(t).max() <= 4017 and np.abs(d).max() < 2 ** 27
    return d


def format_quantise(d, Q):
    """Round half away from zero: sign(d) * ((|d| + (Q << 15)) / (Q << 16)); int64 arrays."""
    return np.sign(d) * ((np.abs(d) + (Q << 15)) // (Q << 16))


def format_coefficients(bgr, quality):
    """The quantised coefficients int64 [mcus, 6, 64] (natural order) the documented format gives a
    BGR24 picture [h, w, 3] at `quality`."""
    q = format_quantise(format_dct(format_samples(bgr)), _quant_blocks(quality))
    q = q.reshape(q.shape[0], 6, 64)
    _assert_no_clamp(q, RESTART_INTERVAL)
    return q


# ------------------------------------------------------------------------- (d) the mathematics

COLOUR_MARGIN = 3 * 255 * 2.0 ** -17  # three products of a coefficient rounded to 16 fraction bits


def float_colour(b, g, r):
    """JFIF: float64 (Y, Cb, Cr)."""
    b, g, r = (np.asarray(v, dtype=np.float64) for v in (b, g, r))
    return (0.299 * r + 0.587 * g + 0.114 * b,
            128.0 - 0.168736 * r - 0.331264 * g + 0.5 * b,
            128.0 + 0.5 * r - 0.418688 * g - 0.081312 * b)


def colour_band(f):
    """(low, high): the sample values the colour rule allows for the float64 value f. They differ
    only where f + 0.5 lies within COLOUR_MARGIN of an integer."""
    return np.floor(f + 0.5 - COLOUR_MARGIN), np.floor(f + 0.5 + COLOUR_MARGIN)


def check_colour(name, got, f):
    """Colour rule: got (integers) against the float64 JFIF values f. Returns the undecidable share."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == np.shape(f)
    assert got.min() >= 0 and got.max() <= 255, f"{name}: value outside 0..255"
    low, high = colour_band(f)
    bad = (got < low) | (got > high)
    share = float((low != high).mean())
    if bad.any():
        i = tuple(int(k) for k in np.argwhere(bad)[0])
        raise AssertionError(f"{name}: {int(bad.sum())} of {bad.size} samples outside the colour rule; first at {i}: "
                             f"got {got[i]:.0f}, JFIF {np.asarray(f)[i]:.6f}")
    return share


def float_samples(bgr):
    """8-bit sample blocks of (d), level-shifted: float64 [mcus, 6, 8, 8]. See the module docstring
    for the undecidable colours."""
    p = replicate(bgr)
    planes = []
    for f, s in zip(float_colour(p[..., 0], p[..., 1], p[..., 2]), format_colour(p[..., 0], p[..., 1], p[..., 2])):
        low, high = colour_band(f)
        assert ((s >= low) & (s <= high)).all(), "the 16.16 formula left the colour rule"
        planes.append(np.where(low == high, np.floor(f + 0.5), s.astype(np.float64)))
    y, cb, cr = planes
    mean = lambda c: np.floor((c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2]) / 4.0 + 0.5)
    return _mcu_blocks(y, mean(cb), mean(cr)) - 128.0


def float_dct(p):
    """float64 [..., 8, 8] real-unit samples -> unquantised coefficients [..., v, u]."""
    return np.einsum("vy,...yx,ux->...vu", C, p, C)


# Measured with this module on the CPU (test_integer_transform_stays_inside_its_bound), luma
# quantisers, 2000 random blocks per kind. noise: uniform 8-bit samples. ramps: a plane with slopes
# up to +-12 levels a sample and a random offset, clipped to 8 bits, so many blocks are partly
# saturated. "error": the largest real error of the documented integer transform against the
# float64 one; "bound": the largest value of bound(); "share": undecidable coefficients under the
# float rule.
#
#   input   quality   error   bound   share
#   noise   1         0.152   0.348   0.14 %
#   noise   25        0.145   0.353   0.83 %
#   noise   50        0.150   0.341   1.61 %
#   noise   85        0.161   0.338   5.51 %    (above the cap: exact rule only)
#   noise   100       0.160   0.341   55.7 %    (exact rule only)
#   ramps   50        0.350   0.530   0.53 %
#   ramps   85        0.353   0.530   2.28 %
#   ramps   95        0.353   0.530   9.50 %    (measured only)
#
# The integer transform never left its bound; the smallest slack was 0.026 (ramps), 0.116 (noise).
# Saturated blocks have the largest sums of |p| and so the largest errors and bounds. So the float
# rule runs on noise at quality 1, 25 and 50 and on smooth pictures at 50 and 85; at quality 100
# and on noise at 85 the format's 3 fraction bits legitimately move coefficients, and only the
# exact rule decides.
#
# Per picture (CASES below; whole pictures, both quantiser tables; the CPU encoder and the kernels
# on an MI355X gave the same figures). "other": undecidable coefficients that took the neighbour of
# round(v); no other coefficient differed anywhere. max |got - v| is the rounding's 0.5 plus what
# the bound allows (b = bound / Q).
#
#   case              quality  share     largest b  max |got - v|  other
#   odd-17x9          1        0.130 %   0.0017     0.4990         0 / 768
#   odd-17x9          25       0.130 %   0.0171     0.5000         0 / 768
#   odd-17x9          50       1.172 %   0.0342     0.5000         1 / 768
#   odd-33x47         25       0.550 %   0.0138     0.5001         1 / 3456
#   odd-33x47         50       0.926 %   0.0275     0.5005         1 / 3456
#   two-intervals     50       0.260 %   0.0252     0.5012         1 / 2304
#   two-intervals     85       0.738 %   0.0860     0.4961         0 / 2304
#   rst-cycle         50       1.117 %   0.0318     0.5057         35 / 39936
#   rst-cycle-smooth  50       0.073 %   0.0412     0.5000         1 / 39936
#   rst-cycle-smooth  85       0.629 %   0.1252     0.5250         15 / 39936
#
# Colour rule over all 2^24 colours: 1.10 % (Y), 1.06 % (Cb), 1.22 % (Cr) undecidable, none outside;
# the 1024 colours of the "colours" case: 0.68 %, 1.66 %, 1.27 %; 442 of the 1024 cells are ties.
def bound(p):
    """Per-coefficient error bound [..., v, u] of the format's integer transform for real-unit
    sample blocks p [..., y, x]; derivation in the module docstring."""
    p = np.asarray(p, dtype=np.float64)
    t = np.einsum("ux,...yx->...yu", C, p)
    eps_t = 2.0 ** -14 * np.abs(p).sum(axis=-1) + 2.0 ** -4  # [..., y]
    return (np.einsum("vy,...y->...v", np.abs(C) + 2.0 ** -14, eps_t)[..., :, None]
            + 2.0 ** -14 * np.abs(t).sum(axis=-2)[..., None, :])


def float_coefficients(bgr, quality):
    """(v, b): oracle (d) divided by the quantiser and the bound divided by the quantiser, both
    float64 [mcus, 6, 64] in natural order."""
    p = float_samples(bgr)
    Q = _quant_blocks(quality).astype(np.float64)
    d = float_dct(p)
    n = d.shape[0]
    rounded = np.sign(d / Q) * np.floor(np.abs(d / Q) + 0.5)
    _assert_no_clamp(rounded.reshape(n, 6, 64).astype(np.int64), RESTART_INTERVAL)
    return (d / Q).reshape(n, 6, 64), (bound(p) / Q).reshape(n, 6, 64)


# ------------------------------------------------------------------------------------- the rules

UNDECIDABLE_CAP = 0.05


def check_exact(name, got, bgr, quality):
    """Exact rule: the coefficients read from a stream equal (c). Every quality, every shape."""
    want = format_coefficients(bgr, quality)
    assert got.shape == want.shape, (got.shape, want.shape)
    bad = got != want
    if bad.any():
        m, b, k = (int(i) for i in np.argwhere(bad)[0])
        raise AssertionError(f"{name} q{quality}: {int(bad.sum())} of {bad.size} coefficients differ from the documented "
                             f"arithmetic; first at MCU {m} block {b} position {k}: got {got[m, b, k]}, want {want[m, b, k]}")


def float_band(v, b):
    """(sign, low, high, share): the magnitudes the float rule allows and the share of undecidable
    coefficients, from the oracle alone. The cap is asserted here, before anything is compared."""
    a = np.abs(v)
    low, high = np.floor(a + 0.5 - b), np.floor(a + 0.5 + b)
    share = float((low != high).mean())
    assert share <= UNDECIDABLE_CAP, f"the oracle leaves {share:.2%} of the coefficients undecidable"
    return np.sign(v), low, high, share


def check_float(name, got, bgr, quality):
    """Float rule: a coefficient equals sign(v) * floor(|v| + 0.5), unless |v| + 0.5 lies within b
    of an integer; then it may take either neighbour. Returns (share, max |got - v|)."""
    v, b = float_coefficients(bgr, quality)
    assert got.shape == v.shape, (got.shape, v.shape)
    sign, low, high, share = float_band(v, b)
    g = got.astype(np.float64)
    err = float(np.abs(g - v).max())
    mag = g * sign
    bad = np.where(sign == 0, g != 0, (mag < low) | (mag > high))
    other = int((g != sign * np.floor(np.abs(v) + 0.5)).sum())
    print(f"{name} q{quality}: undecidable {share:.3%} max|got-v| {err:.4f} largest b {b.max():.4f} "
          f"coefficients != round(v) {other} of {g.size}")
    if bad.any():
        m, blk, k = (int(i) for i in np.argwhere(bad)[0])
        raise AssertionError(f"{name} q{quality}: {int(bad.sum())} of {bad.size} coefficients outside the float rule; first "
                             f"at MCU {m} block {blk} position {k}: got {got[m, blk, k]}, oracle {v[m, blk, k]:.5f} "
                             f"+- {b[m, blk, k]:.5f}")
    return share, err


def constant_samples(name, coefs, blocks):
    """At quality 100 every quantiser is 1 and a constant 8x8 block of samples s codes as
    DC = 8 * (s - 128) with no AC. Returns the samples [mcus, len(blocks)] read back from the DCs
    of the given blocks, after asserting exactly that shape of the coefficients."""
    c = coefs[:, blocks]
    assert not c[:, :, 1:].any(), f"{name}: a constant block has AC coefficients"
    assert not (c[:, :, 0] % 8).any(), f"{name}: the DC of a constant block is no multiple of 8"
    return c[:, :, 0] // 8 + 128


# ------------------------------------------------------------------------ pictures and the cases

def noise(w, h, seed=None):
    return np.random.default_rng(w * 7919 + h if seed is None else seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def gradient(w, h):
    """The gradient of test_gpu_jpeg.picture."""
    yy, xx = np.mgrid[0:h, 0:w]
    return np.stack([xx * 255 // max(w - 1, 1), yy * 255 // max(h - 1, 1), (xx + yy) * 255 // max(w + h - 2, 1)],
                    -1).astype(np.uint8)


def ramps(w, h):
    """Three planes of different slopes, one of them clipped at both ends."""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    b = 5.0 * xx + 1.5 * yy
    g = 250.0 - 3.0 * xx - 4.0 * yy
    r = 40.0 + 7.25 * yy - 2.5 * xx
    return np.clip(np.floor(np.stack([b, g, r], -1)), 0, 255).astype(np.uint8)


def _per_mcu(cells):
    """[32, 32, 2, 2, 3] one 2x2 cell per MCU -> the 512 x 512 picture tiled with them."""
    return np.ascontiguousarray(np.tile(cells, (1, 1, 8, 8, 1)).transpose(0, 2, 1, 3, 4).reshape(512, 512, 3))


def colour_list():
    """1024 BGR colours: the 8 corners, the primaries at 1 and 254, all 256 greys, seeded random."""
    cols = [(b, g, r) for b in (0, 255) for g in (0, 255) for r in (0, 255)]
    for v in (1, 254):
        cols += [(v, 0, 0), (0, v, 0), (0, 0, v)]
    cols += [(s, s, s) for s in range(256)]
    rest = np.random.default_rng(1024).integers(0, 256, (1024 - len(cols), 3))
    return np.concatenate([np.array(cols, dtype=np.int64), rest]).astype(np.uint8)


def colours_picture():
    """(picture, colours [1024, 3]): MCU m of the 512 x 512 picture has the constant colour m."""
    cols = colour_list()
    return _per_mcu(np.broadcast_to(cols.reshape(32, 32, 1, 1, 3), (32, 32, 2, 2, 3))), cols


def cells_picture():
    """(picture, cells [1024, 2, 2, 3]): MCU m is tiled with its own random 2x2 BGR cell."""
    cells = np.random.default_rng(2048).integers(0, 256, (32, 32, 2, 2, 3), dtype=np.uint8)
    return _per_mcu(cells), cells.reshape(1024, 2, 2, 3)


def check_colours(name, coefs, cols):
    """The "colours" picture at quality 100: Y, Cb, Cr of every MCU read back from the DCs and
    held against the float64 JFIF value with the colour rule."""
    s = constant_samples(name, coefs, [0, 1, 2, 3, 4, 5])
    assert (s[:, :4] == s[:, :1]).all(), f"{name}: the four luma blocks of a constant MCU differ"
    f = float_colour(cols[:, 0], cols[:, 1], cols[:, 2])
    shares = [check_colour(f"{name} {c}", s[:, k], f[i]) for i, (c, k) in enumerate((("Y", 0), ("Cb", 4), ("Cr", 5)))]
    print(f"{name}: {len(cols)} colours, undecidable Y {shares[0]:.2%} Cb {shares[1]:.2%} Cr {shares[2]:.2%}")


def check_cells(name, coefs, cells):
    """The "cells" picture at quality 100: the chroma sample of every MCU read back from its DC
    equals the float64 mean of the four converted samples, rounded half up. The four samples are
    those of (d); at least 10 % of the cells must be ties (a sum of the form 4k + 2)."""
    s = constant_samples(name, coefs, [4, 5])
    b, g, r = (cells[..., k].reshape(-1, 4).astype(np.int64) for k in range(3))
    f = float_colour(b, g, r)
    fmt = format_colour(b, g, r)
    tie = np.zeros(len(cells), dtype=bool)
    for k in (1, 2):
        low, high = colour_band(f[k])
        assert ((fmt[k] >= low) & (fmt[k] <= high)).all()
        conv = np.where(low == high, np.floor(f[k] + 0.5), fmt[k].astype(np.float64))
        total = conv.sum(axis=1)
        tie |= (total % 4) == 2
        want = np.floor(total / 4.0 + 0.5)
        bad = s[:, k - 1] != want
        assert not bad.any(), (f"{name}: {int(bad.sum())} chroma means differ; first at MCU {int(np.argmax(bad))}: "
                               f"got {s[int(np.argmax(bad)), k - 1]}, samples {conv[int(np.argmax(bad))]}")
    print(f"{name}: {int(tie.sum())} of {len(cells)} cells are ties")
    assert tie.mean() >= 0.10, "too few ties among the cells"


# id -> (w, h, content, qualities of the exact rule, qualities of the float rule)
CASES = {
    "one-pixel": (1, 1, "noise", (1, 50, 100), ()),
    "odd-17x9": (17, 9, "noise", (1, 25, 50, 85, 100), (1, 25, 50)),
    "odd-33x47": (33, 47, "noise", (25, 50, 100), (25, 50)),
    "two-intervals": (48, 32, "ramps", (50, 85, 100), (50, 85)),
    "rst-cycle": (200, 120, "noise", (50, 100), (50,)),
    "rst-cycle-smooth": (200, 120, "gradient", (50, 85), (50, 85)),
    "colours": (512, 512, "colours", (100,), ()),
    "cells": (512, 512, "cells", (100,), ()),
}
# MCUs and intervals of the cases above at 16 x 16 MCUs and RESTART_INTERVAL = 3 (asserted)
CASE_MCUS = {"one-pixel": (1, 1), "odd-17x9": (2, 1), "odd-33x47": (9, 3), "two-intervals": (6, 2),
             "rst-cycle": (104, 35), "rst-cycle-smooth": (104, 35), "colours": (1024, 342), "cells": (1024, 342)}


def case_picture(case):
    """(picture uint8 [h, w, 3], extra): extra = the colours / cells of those two cases."""
    w, h, content = CASES[case][:3]
    if content == "colours":
        return colours_picture()
    if content == "cells":
        return cells_picture()
    return {"noise": noise, "gradient": gradient, "ramps": ramps}[content](w, h), None


def check_structure(name, st, w, h, quality):
    """What every stream of the encoder shows to the reader."""
    assert (st.w, st.h) == (w, h), f"{name}: SOF0 says {st.w}x{st.h}"
    assert st.sampling == [(2, 2), (1, 1), (1, 1)], f"{name}: sampling {st.sampling}"
    assert st.dri == RESTART_INTERVAL, f"{name}: DRI {st.dri}"
    ql, qc = ijg_tables(quality)
    assert st.tq == [0, 1, 1]
    assert np.array_equal(st.qt[0], ql) and np.array_equal(st.qt[1], qc), f"{name}: DQT is not the IJG rule at q{quality}"
    dedup = [m for k, m in enumerate(st.markers) if k == 0 or st.markers[k - 1] != m]
    assert dedup == [0xD8, 0xE0, 0xDB, 0xC0, 0xC4, 0xDD, 0xDA], [hex(m) for m in st.markers]


def check_case(case, encode):
    """All rules of one case. ``encode(picture, quality) -> bytes`` is the encoder under test.
    Returns [(quality, share, max err)] of the float rule."""
    w, h, content, exact_q, float_q = CASES[case]
    img, extra = case_picture(case)
    assert img.shape == (h, w, 3)
    mcus = -(-w // 16) * -(-h // 16)
    assert (mcus, -(-mcus // RESTART_INTERVAL)) == CASE_MCUS[case], "the case no longer sits where its reason says"
    out = []
    for q in exact_q:
        st = read_stream(encode(img, q))
        check_structure(case, st, w, h, q)
        assert st.coefs.shape == (mcus, 6, 64)
        assert st.interval_mcus == [min(3, mcus - 3 * k) for k in range(-(-mcus // 3))]
        check_exact(case, st.coefs, img, q)
        if q in float_q:
            out.append((q,) + check_float(case, st.coefs, img, q))
        if content == "colours":
            check_colours(case, st.coefs, extra)
        if content == "cells":
            check_cells(case, st.coefs, extra)
    assert set(float_q) <= set(exact_q)
    return out
