"""Tensor-level ops backed by the gfx950 HIP kernels (and their plain-PyTorch references).

* :func:`nv12_to_bgr` — BT.601 limited-range NV12 -> packed BGR24 (the kernel behind
  ``VideoFrame.data``; reference: python/read_image.py:94 ``to_ndarray(format='bgr24')``).
* :func:`surface_to_bgr` / :func:`surface_to_bgr_batch` — a reconstructed surface at its native
  sample format (uint8 / uint16 samples, 4:2:0 / 4:2:2) -> BGR24, narrowed in registers (the
  frame history's conversion; one launch for several pictures).
* :func:`pcm_decode_bgr` — fused I_PCM macroblock reconstruction + conversion.
* :func:`letterbox` — NV12 -> letterboxed model input (HWC uint8 and/or normalised CHW).
* :func:`jpeg_encode` — BGR24 picture -> baseline JPEG stream (the kernels behind ``frame.jpg``),
  byte-identical with :func:`jpeg_encode_reference`, the CPU encoder.
* :func:`resize_area` / :func:`compose_wall` — antialiased area-average downscale of BGR24
  pictures, one or many into one canvas in a single launch (the kernel behind scaled
  ``frame.jpg`` and ``wall.jpg``), byte-identical with their ``*_reference`` CPU twins.
* :func:`motion_update` / :func:`motion_update_batch` — a BGR24 picture against a running
  background model: changed pixels per cell and the updated model, one or many pictures in a
  single launch (the kernel behind ``/motion``), byte-identical with
  :func:`motion_update_reference`.
* :func:`tamper_stats` / :func:`tamper_stats_batch` — the luma histogram, per-cell luma sums and
  per-cell focus energy of BGR24 pictures, one or many in a single launch (the kernel behind
  ``/tamper``), byte-identical with :func:`tamper_stats_reference`.
* :func:`privacy_mask` / :func:`privacy_mask_batch` — fill or pixelate rectangles of BGR24
  pictures in place, one launch per level of overlap for all pictures (the kernel that masks a
  camera's ring slot before it is published), byte-identical with :func:`privacy_mask_reference`.
* :func:`crop_resize` / :func:`crop_resize_batch` — boxes of BGR24 pictures cut and resized
  (reduced by area averaging, enlarged bilinearly, stretched or letterboxed) to one output size,
  every box of every picture in a single launch (the kernel behind ``/crops`` and ``crop.jpg``),
  byte-identical with :func:`crop_resize_reference`.

The ``*_reference`` functions are the fp32 PyTorch oracles the GPU tests compare against.
Calling a GPU op on a host with no HIP device raises (no silent CPU fallback).
"""
from __future__ import annotations

import torch

from .._native import native, require_gpu

_CHW_DTYPES = {None: 0, torch.float16: 1, torch.bfloat16: 2, torch.float32: 3}


def _stream_ptr(t: torch.Tensor) -> int:
    return int(torch.cuda.current_stream(t.device).cuda_stream)


def _check_nv12(y: torch.Tensor, uv: torch.Tensor):
    if not (y.is_cuda and uv.is_cuda):
        raise ValueError("nv12 planes must be device tensors")
    if y.dtype != torch.uint8 or uv.dtype != torch.uint8:
        raise TypeError("nv12 planes must be uint8")
    if not (y.is_contiguous() and uv.is_contiguous()):
        raise ValueError("nv12 planes must be contiguous")
    H, W = y.shape
    if W % 16 or H % 16:
        raise ValueError("coded NV12 size must be macroblock aligned (multiple of 16)")
    if tuple(uv.shape) != (H // 2, W):
        raise ValueError(f"uv plane must be {(H // 2, W)}, got {tuple(uv.shape)}")
    return H, W


def nv12_to_bgr(y: torch.Tensor, uv: torch.Tensor, width: int | None = None,
                height: int | None = None, crop_left: int = 0, crop_top: int = 0,
                out: torch.Tensor | None = None) -> torch.Tensor:
    """Convert a macroblock-aligned NV12 surface to a ``[height, width, 3]`` BGR24 tensor."""
    require_gpu()
    H, W = _check_nv12(y, uv)
    width = W - crop_left if width is None else width
    height = H - crop_top if height is None else height
    if out is None:
        out = torch.empty((height, width, 3), dtype=torch.uint8, device=y.device)
    assert out.is_contiguous() and tuple(out.shape) == (height, width, 3)
    native.nv12_to_bgr(y.data_ptr(), uv.data_ptr(), 0, 0, 0, 0, W // 16, H // 16, width,
                       height, crop_left, crop_top, out.data_ptr(), _stream_ptr(y))
    return out


def _surface_args(y: torch.Tensor, uv: torch.Tensor, bit_depth: int, chroma_format: int,
                  width, height, crop_left: int, crop_top: int, out):
    if not (y.is_cuda and uv.is_cuda):
        raise ValueError("surface planes must be device tensors")
    want = torch.uint8 if bit_depth == 8 else torch.uint16
    if bit_depth not in (8, 9, 10):
        raise ValueError("bit_depth must be 8, 9 or 10")
    if y.dtype != want or uv.dtype != want:
        raise TypeError(f"{bit_depth}-bit surface planes must be {want}")
    if chroma_format not in (1, 2):
        raise ValueError("chroma_format must be 1 (4:2:0) or 2 (4:2:2)")
    if not (y.is_contiguous() and uv.is_contiguous()):
        raise ValueError("surface planes must be contiguous")
    H, W = y.shape
    if W % 16 or H % 16:
        raise ValueError("coded surface size must be macroblock aligned (multiple of 16)")
    ch = H if chroma_format == 2 else H // 2
    if tuple(uv.shape) != (ch, W):
        raise ValueError(f"uv plane must be {(ch, W)}, got {tuple(uv.shape)}")
    width = W - crop_left if width is None else width
    height = H - crop_top if height is None else height
    if crop_left < 0 or crop_top < 0 or width <= 0 or height <= 0 or crop_left + width > W or crop_top + height > H:
        raise ValueError("output window outside the coded picture")
    if out is None:
        out = torch.empty((height, width, 3), dtype=torch.uint8, device=y.device)
    if not (out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous() and tuple(out.shape) == (height, width, 3)):
        raise ValueError(f"out must be a contiguous uint8 device tensor of shape {(height, width, 3)}")
    return (y.data_ptr(), uv.data_ptr(), W, W, H, bit_depth, chroma_format, crop_left, crop_top, width, height,
            out.data_ptr()), out


def surface_to_bgr(y: torch.Tensor, uv: torch.Tensor, bit_depth: int = 8, chroma_format: int = 1,
                   width: int | None = None, height: int | None = None, crop_left: int = 0,
                   crop_top: int = 0, out: torch.Tensor | None = None) -> torch.Tensor:
    """Convert a reconstructed surface at its native sample format to ``[height, width, 3]``
    BGR24: uint8 planes (``bit_depth`` 8) or uint16 planes (9..10, rounded to 8 bits), chroma
    4:2:0 (``uv`` of H/2 rows) or 4:2:2 (H rows, row pairs averaged). Bit-exact with the CPU
    reference (narrow_surface + nv12_to_bgr_cpu)."""
    require_gpu()
    args, out = _surface_args(y, uv, bit_depth, chroma_format, width, height, crop_left, crop_top, out)
    native.surface_to_bgr(*args, _stream_ptr(y))
    return out


def surface_to_bgr_batch(pictures) -> list:
    """Convert several surfaces in one kernel launch. ``pictures``: dicts of the keyword arguments
    of :func:`surface_to_bgr` (``y`` and ``uv`` required). Returns the outputs in order."""
    require_gpu()
    pics, outs = [], []
    for p in pictures:
        args, out = _surface_args(p["y"], p["uv"], p.get("bit_depth", 8), p.get("chroma_format", 1), p.get("width"),
                                  p.get("height"), p.get("crop_left", 0), p.get("crop_top", 0), p.get("out"))
        pics.append(args)
        outs.append(out)
    if pics:
        native.surface_to_bgr_many(pics, _stream_ptr(pictures[0]["y"]))
    return outs


def mb_mask_prefix(mb_slot: torch.Tensor):
    """Dense per-MB slot map -> (coded-MB bitmask words, exclusive per-word popcount prefix,
    raster-order permutation of the payload slots) — the compact form the kernel consumes."""
    s = mb_slot.detach().to("cpu", torch.int64)
    n = s.numel()
    words = (n + 31) // 32
    coded = torch.zeros(words * 32, dtype=torch.int64)
    coded[:n] = (s >= 0).to(torch.int64)
    bits = coded.view(words, 32) << torch.arange(32, dtype=torch.int64)
    mask = bits.sum(1)
    counts = coded.view(words, 32).sum(1)
    prefix = torch.cumsum(counts, 0) - counts
    order = s[s >= 0]
    to_i32 = lambda t: torch.where(t >= 2**31, t - 2**32, t).to(torch.int32)
    return to_i32(mask), prefix.to(torch.int32), order


def pcm_decode_bgr(y: torch.Tensor, uv: torch.Tensor, mb_slot: torch.Tensor,
                   payload: torch.Tensor, width: int | None = None,
                   height: int | None = None) -> torch.Tensor:
    """Apply I_PCM macroblocks (``mb_slot[mb]`` -> 384-byte slot in ``payload``, -1 = keep) to
    the NV12 surface in place and return the converted BGR24 picture."""
    require_gpu()
    H, W = _check_nv12(y, uv)
    if mb_slot.dtype != torch.int32 or mb_slot.numel() != (H // 16) * (W // 16):
        raise ValueError("mb_slot must be int32 with one entry per macroblock")
    if payload.dtype != torch.uint8 or payload.numel() % 384:
        raise ValueError("payload must be uint8 with 384-byte slots")
    nslots = payload.numel() // 384
    if nslots and int(mb_slot.max().item()) >= nslots:
        raise ValueError("mb_slot references a payload slot out of range")
    width = W if width is None else width
    height = H if height is None else height
    mask, prefix, order = mb_mask_prefix(mb_slot)
    offsets = (order * 384).to(torch.int32).to(y.device)  # samples read in place from payload
    mask, prefix = mask.to(y.device), prefix.to(y.device)
    payload = payload.to(y.device).contiguous()
    out = torch.empty((height, width, 3), dtype=torch.uint8, device=y.device)
    native.nv12_to_bgr(y.data_ptr(), uv.data_ptr(), mask.data_ptr(), prefix.data_ptr(),
                       offsets.data_ptr(), payload.data_ptr(), W // 16, H // 16, width, height,
                       0, 0, out.data_ptr(), _stream_ptr(y))
    torch.cuda.current_stream(y.device).synchronize()  # host-built index tensors go out of scope
    return out


def letterbox_geometry(src_w: int, src_h: int, size: int, even: bool = False):
    """(new_w, new_h, pad_x, pad_y) of the centred aspect-preserving fit (even: NV12-aligned)."""
    return tuple(native.letterbox_geometry(src_w, src_h, size, even))


def _check_letterbox(y: torch.Tensor, uv: torch.Tensor, size: int, width, height, crop_left: int,
                     crop_top: int):
    """Shared argument checks of the letterbox ops: the kernels read the window
    ``[crop_top, crop_top + height) x [crop_left, crop_left + width)`` of the planes unchecked."""
    H, W = _check_nv12(y, uv)
    width = W - crop_left if width is None else width
    height = H - crop_top if height is None else height
    if size <= 0 or size % 8:
        raise ValueError("size must be a positive multiple of 8")
    if width <= 0 or height <= 0:
        raise ValueError("width and height must be positive")
    if crop_left < 0 or crop_top < 0 or crop_left + width > W or crop_top + height > H:
        raise ValueError("source window outside the coded picture")
    return W, int(width), int(height)


def letterbox_nv12(y: torch.Tensor, uv: torch.Tensor, size: int = 640, width: int | None = None,
                   height: int | None = None, crop_left: int = 0, crop_top: int = 0,
                   pad_value: int = 114) -> torch.Tensor:
    """NV12 -> letterboxed NV12 ``[S*S*3/2]`` uint8 (Y and UV planes resized independently):
    the compact consumer format that crosses xGMI in the all-gather."""
    require_gpu()
    W, width, height = _check_letterbox(y, uv, size, width, height, crop_left, crop_top)
    out = torch.empty((size * size * 3 // 2,), dtype=torch.uint8, device=y.device)
    native.letterbox(y.data_ptr(), uv.data_ptr(), W, width, height, crop_left, crop_top, size,
                     out.data_ptr(), 0, 0, [0.0] * 3, [1.0] * 3, int(pad_value), _stream_ptr(y), 1)
    return out


def nv12_to_chw(batch: torch.Tensor, size: int, dtype: torch.dtype = torch.bfloat16,
                mean=(0.0, 0.0, 0.0), std=(1.0, 1.0, 1.0)) -> torch.Tensor:
    """Consumer-side: ``[N, S*S*3/2]`` NV12 batch -> ``[N, 3, S, S]`` normalised RGB (BT.601)."""
    require_gpu()
    if batch.dtype != torch.uint8 or not batch.is_contiguous():
        raise ValueError("batch must be contiguous uint8")
    if size <= 0 or size % 4:
        raise ValueError("size must be a positive multiple of 4")
    if _CHW_DTYPES.get(dtype, 0) == 0:
        raise TypeError("dtype must be float16, bfloat16 or float32")
    if any(float(s) == 0.0 for s in std):
        raise ValueError("std must not contain 0")
    n = batch.numel() // (size * size * 3 // 2)
    if n * size * size * 3 // 2 != batch.numel():
        raise ValueError("batch size is not a whole number of S x S NV12 pictures")
    out = torch.empty((n, 3, size, size), dtype=dtype, device=batch.device)
    native.nv12_to_chw(batch.data_ptr(), out.data_ptr(), n, size, _CHW_DTYPES[dtype],
                       list(map(float, mean)), list(map(float, std)), _stream_ptr(batch))
    return out


def letterbox_nv12_reference(y: torch.Tensor, uv: torch.Tensor, size: int, width: int,
                             height: int, pad_value: int = 114) -> torch.Tensor:
    """fp32 torch reference of :func:`letterbox_nv12` (per-plane bilinear, align_corners=False).

    Both planes are sampled with the luma ratios ``width / nw`` and ``height / nh``: the chroma
    plane of a picture covers ``width / 2`` chroma samples of picture (also when ``width`` is odd
    and the plane stores ``(width + 1) // 2``), so its scale is the luma's, not the ratio of the
    stored plane sizes an ``F.interpolate`` call would derive."""
    nw, nh, px, py = letterbox_geometry(width, height, size, even=True)
    rx = torch.tensor(float(width), dtype=torch.float32) / float(nw)
    ry = torch.tensor(float(height), dtype=torch.float32) / float(nh)

    def axis(n, r, src):
        s = ((torch.arange(n, dtype=torch.float32) + 0.5) * r - 0.5).clamp(min=0.0)
        i0 = s.floor().long().clamp(max=src - 1)
        return i0.to(y.device), (i0 + 1).clamp(max=src - 1).to(y.device), (s - i0.float()).to(y.device)

    def resize(P, oh, ow):  # P: [..., h, w] float32
        y0, y1, ly = axis(oh, ry, P.shape[-2])
        x0, x1, lx = axis(ow, rx, P.shape[-1])
        ly = ly[:, None]
        top = (1 - lx) * P[..., y0, :][..., x0] + lx * P[..., y0, :][..., x1]
        bot = (1 - lx) * P[..., y1, :][..., x0] + lx * P[..., y1, :][..., x1]
        return (1 - ly) * top + ly * bot

    ypad = round(16 + pad_value * 219 / 255)
    yo = torch.full((size, size), float(ypad), device=y.device)
    yo[py:py + nh, px:px + nw] = resize(y[:height, :width].float(), nh, nw)
    cw, chh = (width + 1) // 2, (height + 1) // 2
    C = uv[:chh, :cw * 2].float().view(chh, cw, 2).permute(2, 0, 1)
    co = torch.full((2, size // 2, size // 2), 128.0, device=y.device)
    co[:, py // 2:py // 2 + nh // 2, px // 2:px // 2 + nw // 2] = resize(C, nh // 2, nw // 2)
    out_y = (yo + 0.5).clamp(0, 255).floor().to(torch.uint8).flatten()
    out_c = (co + 0.5).clamp(0, 255).floor().to(torch.uint8).permute(1, 2, 0).flatten()
    return torch.cat([out_y, out_c])


def letterbox(y: torch.Tensor, uv: torch.Tensor, size: int = 640, width: int | None = None,
              height: int | None = None, crop_left: int = 0, crop_top: int = 0,
              chw_dtype: torch.dtype | None = None, mean=(0.0, 0.0, 0.0), std=(1.0, 1.0, 1.0),
              pad_value: int = 114, hwc: bool = True):
    """NV12 -> (hwc uint8 [S,S,3] BGR or None, chw [3,S,S] RGB normalised or None)."""
    require_gpu()
    W, width, height = _check_letterbox(y, uv, size, width, height, crop_left, crop_top)
    if chw_dtype not in _CHW_DTYPES:
        raise TypeError("chw_dtype must be None, float16, bfloat16 or float32")
    mean, std = list(map(float, mean)), list(map(float, std))
    if len(mean) != 3 or len(std) != 3:
        raise ValueError("mean and std must have three values (RGB)")
    if any(s == 0.0 for s in std):
        raise ValueError("std must not contain 0")
    if not hwc and chw_dtype is None:
        raise ValueError("nothing to compute: hwc is False and chw_dtype is None")
    out_hwc = torch.empty((size, size, 3), dtype=torch.uint8, device=y.device) if hwc else None
    out_chw = (torch.empty((3, size, size), dtype=chw_dtype, device=y.device)
               if chw_dtype is not None else None)
    native.letterbox(y.data_ptr(), uv.data_ptr(), W, width, height, crop_left, crop_top, size,
                     out_hwc.data_ptr() if out_hwc is not None else 0,
                     out_chw.data_ptr() if out_chw is not None else 0,
                     _CHW_DTYPES[chw_dtype], mean, std, int(pad_value), _stream_ptr(y))
    return out_hwc, out_chw


def _check_jpeg(bgr: torch.Tensor, quality: int) -> int:
    if bgr.dtype != torch.uint8:
        raise TypeError("bgr must be uint8")
    if bgr.dim() != 3 or bgr.shape[2] != 3 or bgr.shape[0] < 1 or bgr.shape[1] < 1:
        raise ValueError(f"bgr must be [H, W, 3], got {tuple(bgr.shape)}")
    if bgr.shape[0] > 65535 or bgr.shape[1] > 65535:
        raise ValueError("a JPEG picture is at most 65535 x 65535")
    if not bgr.is_contiguous():
        raise ValueError("bgr must be contiguous")
    if isinstance(quality, bool) or not isinstance(quality, int) or not 1 <= quality <= 100:
        raise ValueError("quality must be an integer 1..100")
    return quality


def jpeg_encode(bgr: torch.Tensor, quality: int = 85) -> bytes:
    """Encode a ``[H, W, 3]`` BGR24 device tensor as a baseline JPEG (JFIF, 4:2:0, restart
    intervals) on the GPU; only the compressed bytes are copied to the host."""
    require_gpu()
    if not bgr.is_cuda:
        raise ValueError("bgr must be a device tensor")
    quality = _check_jpeg(bgr, quality)
    with torch.cuda.device(bgr.device):
        return native.jpeg_encode(bgr.data_ptr(), int(bgr.shape[1]), int(bgr.shape[0]), quality, _stream_ptr(bgr))


def jpeg_encode_reference(bgr: torch.Tensor, quality: int = 85) -> bytes:
    """The CPU encoder's stream of the same picture (host or device tensor): the byte-exact
    oracle of :func:`jpeg_encode`."""
    quality = _check_jpeg(bgr, quality)
    return native.jpeg_encode_cpu(bgr.detach().cpu().numpy(), quality)


def _check_bgr(bgr: torch.Tensor, what: str = "bgr") -> tuple:
    if bgr.dtype != torch.uint8:
        raise TypeError(f"{what} must be uint8")
    if bgr.dim() != 3 or bgr.shape[2] != 3 or bgr.shape[0] < 1 or bgr.shape[1] < 1:
        raise ValueError(f"{what} must be [H, W, 3], got {tuple(bgr.shape)}")
    if bgr.shape[0] > 65535 or bgr.shape[1] > 65535:
        raise ValueError(f"{what} is at most 65535 x 65535")
    if not bgr.is_contiguous():
        raise ValueError(f"{what} must be contiguous")
    return int(bgr.shape[1]), int(bgr.shape[0])


def _check_side(v, what: str) -> int:
    if isinstance(v, bool) or not isinstance(v, int) or not 1 <= v <= 65535:
        raise ValueError(f"{what} must be an integer 1..65535")
    return v


def _check_resize(bgr: torch.Tensor, width: int, height: int):
    sw, sh = _check_bgr(bgr)
    width, height = _check_side(width, "width"), _check_side(height, "height")
    if width > sw or height > sh:
        raise ValueError(f"output {width}x{height} larger than the source {sw}x{sh} (no upscaling)")
    return sw, sh, width, height


def resize_area(bgr: torch.Tensor, width: int, height: int, out: torch.Tensor | None = None) -> torch.Tensor:
    """Downscale a ``[H, W, 3]`` BGR24 device tensor to exactly ``[height, width, 3]`` by area
    averaging (antialiased, exact in integers), byte-identical with :func:`resize_area_reference`."""
    require_gpu()
    if not bgr.is_cuda:
        raise ValueError("bgr must be a device tensor")
    sw, sh, width, height = _check_resize(bgr, width, height)
    if out is None:
        out = torch.empty((height, width, 3), dtype=torch.uint8, device=bgr.device)
    if not (out.is_cuda and out.device == bgr.device and out.dtype == torch.uint8 and out.is_contiguous()
            and tuple(out.shape) == (height, width, 3)):
        raise ValueError(f"out must be a contiguous uint8 tensor of shape {(height, width, 3)} on the source's device")
    with torch.cuda.device(bgr.device):
        native.compose_wall([(bgr.data_ptr(), sw, sh)], -1, width, height, out.data_ptr(), _stream_ptr(bgr))
    return out


def resize_area_reference(bgr: torch.Tensor, width: int, height: int) -> torch.Tensor:
    """The CPU implementation's result for the same picture (host or device tensor), on the host:
    the byte-exact oracle of :func:`resize_area`."""
    _, _, width, height = _check_resize(bgr, width, height)
    return torch.from_numpy(native.resize_area_cpu(bgr.detach().cpu().numpy(), width, height))


def _check_wall(frames, cols, tile_width, tile_height):
    frames = list(frames)
    if not frames:
        raise ValueError("frames must hold at least one tile")
    tile_width, tile_height = _check_side(tile_width, "tile_width"), _check_side(tile_height, "tile_height")
    if cols is None:
        cols = 0
    if isinstance(cols, bool) or not isinstance(cols, int) or not 0 <= cols <= 65535:
        raise ValueError("cols must be an integer 1..65535 (or None)")
    for k, f in enumerate(frames):
        if f is not None:
            _check_bgr(f, f"frames[{k}]")
    gc, gr, cw, ch = native.wall_geometry(len(frames), cols, tile_width, tile_height)
    if cw > 65535 or ch > 65535:
        raise ValueError(f"canvas {cw}x{ch} larger than 65535")
    return frames, cols, tile_width, tile_height, (ch, cw, 3)


def compose_wall(frames, cols: int | None, tile_width: int, tile_height: int,
                 out: torch.Tensor | None = None) -> torch.Tensor:
    """One canvas of several pictures in one kernel launch: ``frames`` is a list of ``[H, W, 3]``
    BGR24 device tensors (any sizes) or ``None`` (an empty tile). Tile ``t`` is fitted into cell
    ``(t % cols, t // cols)`` of ``tile_width x tile_height`` and centred; everything else is
    BGR (16, 16, 16). ``cols`` None: ``ceil(sqrt(n))``. Byte-identical with
    :func:`compose_wall_reference`."""
    require_gpu()
    frames, cols, tile_width, tile_height, shape = _check_wall(frames, cols, tile_width, tile_height)
    device = None
    for f in frames:
        if f is None:
            continue
        if not f.is_cuda:
            raise ValueError("frames must be device tensors")
        if device is None:
            device = f.device
        elif f.device != device:
            raise ValueError("frames must live on one device")
    if device is None:
        device = out.device if out is not None else torch.device("cuda", torch.cuda.current_device())
    if out is None:
        out = torch.empty(shape, dtype=torch.uint8, device=device)
    if not (out.is_cuda and out.device == device and out.dtype == torch.uint8 and out.is_contiguous()
            and tuple(out.shape) == shape):
        raise ValueError(f"out must be a contiguous uint8 tensor of shape {shape} on the frames' device")
    tiles = [(0, 0, 0) if f is None else (f.data_ptr(), int(f.shape[1]), int(f.shape[0])) for f in frames]
    with torch.cuda.device(device):
        native.compose_wall(tiles, cols, tile_width, tile_height, out.data_ptr(), _stream_ptr(out))
    return out


def compose_wall_reference(frames, cols: int | None, tile_width: int, tile_height: int) -> torch.Tensor:
    """The CPU implementation's canvas of the same tiles (host or device tensors), on the host:
    the byte-exact oracle of :func:`compose_wall`."""
    frames, cols, tile_width, tile_height, _ = _check_wall(frames, cols, tile_width, tile_height)
    host = [None if f is None else f.detach().cpu().numpy() for f in frames]
    return torch.from_numpy(native.compose_wall_cpu(host, cols, tile_width, tile_height))


def _check_motion_params(cell, threshold, learn_shift):
    for v, what, lo, hi in ((cell, "cell", 4, 256), (threshold, "threshold", 0, 255), (learn_shift, "learn_shift", 0, 8)):
        if isinstance(v, bool) or not isinstance(v, int) or not lo <= v <= hi:
            raise ValueError(f"{what} must be an integer {lo}..{hi}")
    return cell, threshold, learn_shift


def _check_background(bg: torch.Tensor, w: int, h: int, what: str = "background"):
    if bg.dtype != torch.uint16:
        raise TypeError(f"{what} must be uint16")
    if bg.dim() != 2 or tuple(bg.shape) != (h, w):
        raise ValueError(f"{what} must be [H, W] = {(h, w)}, got {tuple(bg.shape)}")


def _plane_in_place(bg: torch.Tensor) -> bool:
    """The kernel can use the tensor's memory as it lies: samples contiguous in a row, rows a
    multiple of 8 samples apart and 16-byte aligned."""
    h, w = bg.shape
    pitch = bg.stride(0) if h > 1 else native.motion_pitch(w)
    if not ((bg.stride(1) == 1 or w == 1) and pitch % 8 == 0 and pitch >= w and bg.data_ptr() % 16 == 0):
        return False
    # the last group of a row is loaded whole: the last row's padding must be memory of the tensor
    last = bg.storage_offset() + (h - 1) * pitch + native.motion_pitch(w)
    return bg.untyped_storage().nbytes() >= last * 2


def _padded_plane(w: int, h: int, device) -> torch.Tensor:
    return torch.empty((h, native.motion_pitch(w)), dtype=torch.uint16, device=device)


def motion_update_batch(pictures, cell: int = 16, threshold: int = 24, learn_shift: int = 4):
    """One kernel launch for a list of pictures of any sizes on one device. Each entry is ``bgr``,
    ``(bgr, background)`` or ``(bgr, background, out)`` as in :func:`motion_update`; returns the
    list of ``(counts, background)``."""
    require_gpu()
    cell, threshold, learn_shift = _check_motion_params(cell, threshold, learn_shift)
    pictures = list(pictures)
    if not pictures:
        raise ValueError("pictures must hold at least one picture")
    device, work, results, copies = None, [], [], []
    keep = []  # padded copies of the inputs stay alive until the launch is done
    for k, p in enumerate(pictures):
        bgr, bg, out = (tuple(p) + (None, None))[:3] if isinstance(p, (tuple, list)) else (p, None, None)
        w, h = _check_bgr(bgr, f"pictures[{k}]")
        if not bgr.is_cuda:
            raise ValueError("bgr must be a device tensor")
        if device is None:
            device = bgr.device
        for t, what in ((bgr, "bgr"), (bg, "background"), (out, "out")):
            if t is not None and (not t.is_cuda or t.device != device):
                raise ValueError(f"{what} must live on the pictures' device")
        if bg is not None:
            _check_background(bg, w, h)
        if out is not None:
            _check_background(out, w, h, "out")
            if bg is not None and out.data_ptr() == bg.data_ptr():
                raise ValueError("out must not be the background itself (the update is out of place)")
        dst = out if out is not None and _plane_in_place(out) else _padded_plane(w, h, device)[:, :w]
        if out is not None and dst is not out:
            copies.append((out, dst))
        # one pitch for both planes: the output's
        pitch = int(dst.stride(0)) if h > 1 else native.motion_pitch(w)
        src = 0
        if bg is not None:
            if not (_plane_in_place(bg) and (h == 1 or bg.stride(0) == pitch)):
                pad = torch.empty((h, pitch), dtype=torch.uint16, device=device)
                pad[:, :w].copy_(bg)
                bg = pad[:, :w]
                keep.append(pad)
            src = bg.data_ptr()
        cols, rows = native.motion_grid(w, h, cell)
        counts = torch.empty((rows, cols), dtype=torch.int32, device=device)
        work.append((bgr.data_ptr(), w, h, src, dst.data_ptr(), pitch, counts.data_ptr()))
        keep.append(dst)
        results.append((counts, out if out is not None else dst))
    with torch.cuda.device(device):
        native.motion_update(work, cell, threshold, learn_shift, int(torch.cuda.current_stream(device).cuda_stream))
    for out, dst in copies:
        out.copy_(dst)
    return results


def motion_update(bgr: torch.Tensor, background: torch.Tensor | None = None, cell: int = 16, threshold: int = 24,
                  learn_shift: int = 4, out: torch.Tensor | None = None):
    """One motion evaluation of a ``[H, W, 3]`` BGR24 device tensor against ``background``, a
    ``[H, W]`` ``torch.uint16`` plane in 8.8 fixed point (``None``: prime): ``(counts, background')``
    with ``counts`` the ``[rows, cols]`` int32 grid of changed pixels per ``cell x cell`` cell and
    ``background'`` the updated plane (``out`` if given, else a new tensor whose rows are padded to a
    multiple of 8 samples). A plane whose row stride is a multiple of 8 samples and whose memory is
    16-byte aligned is used where it lies; any other is copied to and from such a plane. Exact in
    integers, byte-identical with :func:`motion_update_reference`. No CPU fallback."""
    return motion_update_batch([(bgr, background, out)], cell, threshold, learn_shift)[0]


def motion_update_reference(bgr: torch.Tensor, background: torch.Tensor | None = None, cell: int = 16,
                            threshold: int = 24, learn_shift: int = 4):
    """The CPU implementation's result for the same picture (host or device tensors), on the host:
    the byte-exact oracle of :func:`motion_update`."""
    cell, threshold, learn_shift = _check_motion_params(cell, threshold, learn_shift)
    w, h = _check_bgr(bgr)
    bg = None
    if background is not None:
        _check_background(background, w, h)
        bg = background.detach().cpu().contiguous().numpy()
    counts, new = native.motion_update_cpu(bgr.detach().cpu().numpy(), bg, cell, threshold, learn_shift)
    return torch.from_numpy(counts.astype("int32")), torch.from_numpy(new)


def _check_tamper_cell(cell):
    if isinstance(cell, bool) or not isinstance(cell, int) or not 8 <= cell <= 128:
        raise ValueError("cell must be an integer 8..128")
    return cell


def _u32(t: torch.Tensor) -> torch.Tensor:
    """An int32 tensor of u32 bit patterns as int64 values."""
    return t.to(torch.int64) & 0xFFFFFFFF


def tamper_stats_batch(pictures, cell: int = 32, out=None):
    """One kernel launch for a list of ``[H, W, 3]`` BGR24 device tensors of any sizes on one
    device: the list of ``(hist, sum_y, energy)`` of :func:`tamper_stats`. ``out``: ``None`` or one
    ``(hist, sum_y, energy)`` triple of contiguous int32 device tensors per picture, ``[256]``,
    ``[rows, cols]`` and ``[rows, cols]``, which the kernel writes where they lie (as u32 bit
    patterns; the histograms are zeroed on the stream first)."""
    require_gpu()
    cell = _check_tamper_cell(cell)
    pictures = list(pictures)
    if not pictures:
        raise ValueError("pictures must hold at least one picture")
    if out is not None:
        out = list(out)
        if len(out) != len(pictures):
            raise ValueError("out must hold one (hist, sum_y, energy) per picture")
    device, work, raw = None, [], []
    for k, bgr in enumerate(pictures):
        w, h = _check_bgr(bgr, f"pictures[{k}]")
        if not bgr.is_cuda:
            raise ValueError("bgr must be a device tensor")
        if device is None:
            device = bgr.device
        if bgr.device != device:
            raise ValueError("the pictures must live on one device")
        cols, rows = native.tamper_grid(w, h, cell)
        if out is None:
            bufs = (torch.empty(256, dtype=torch.int32, device=device),
                    torch.empty((rows, cols), dtype=torch.int32, device=device),
                    torch.empty((rows, cols), dtype=torch.int32, device=device))
        else:
            bufs = tuple(out[k])
            if len(bufs) != 3:
                raise ValueError("out must hold one (hist, sum_y, energy) per picture")
            for t, shape, what in zip(bufs, ((256,), (rows, cols), (rows, cols)), ("hist", "sum_y", "energy")):
                if not isinstance(t, torch.Tensor) or t.dtype != torch.int32:
                    raise TypeError(f"out[{k}] {what} must be an int32 tensor")
                if tuple(t.shape) != shape or not t.is_contiguous():
                    raise ValueError(f"out[{k}] {what} must be contiguous {shape}, got {tuple(t.shape)}")
                if not t.is_cuda or t.device != device:
                    raise ValueError(f"out[{k}] {what} must live on the pictures' device")
        work.append((bgr.data_ptr(), w, h, bufs[0].data_ptr(), bufs[1].data_ptr(), bufs[2].data_ptr()))
        raw.append(bufs)
    with torch.cuda.device(device):
        native.tamper_stats(work, cell, int(torch.cuda.current_stream(device).cuda_stream))
    return [tuple(_u32(t) for t in bufs) for bufs in raw]


def tamper_stats(bgr: torch.Tensor, cell: int = 32, out=None):
    """The tamper statistics of a ``[H, W, 3]`` BGR24 device tensor (csrc/vep/tamper.h):
    ``(hist, sum_y, energy)`` with ``hist`` the ``[256]`` luma histogram, ``sum_y`` the
    ``[rows, cols]`` luma sums of the ``cell x cell`` cells and ``energy`` their squared-gradient
    focus measure. All three are ``torch.int64``: the kernel's values are u32 (a bin holds up to
    65535² pixels, above int32), and int64 holds that range without a sign. Exact in integers,
    byte-identical with :func:`tamper_stats_reference`. No CPU fallback."""
    return tamper_stats_batch([bgr], cell, None if out is None else [out])[0]


def tamper_stats_reference(bgr: torch.Tensor, cell: int = 32):
    """The CPU implementation's result for the same picture (host or device tensor), on the host:
    the byte-exact oracle of :func:`tamper_stats`, int64 like it."""
    cell = _check_tamper_cell(cell)
    _check_bgr(bgr)
    return tuple(torch.from_numpy(a.astype("int64")) for a in native.tamper_stats_cpu(bgr.detach().cpu().numpy(), cell))


def _check_mask_picture(bgr, what: str = "bgr") -> tuple:
    if not isinstance(bgr, torch.Tensor) or bgr.dtype != torch.uint8:
        raise ValueError(f"{what} must be a uint8 tensor")
    if bgr.dim() != 3 or bgr.shape[2] != 3 or bgr.shape[0] < 1 or bgr.shape[1] < 1:
        raise ValueError(f"{what} must be [H, W, 3], got {tuple(bgr.shape)}")
    if bgr.shape[0] > 65535 or bgr.shape[1] > 65535:
        raise ValueError(f"{what} is at most 65535 x 65535")
    if not bgr.is_contiguous():
        raise ValueError(f"{what} must be contiguous")
    return int(bgr.shape[1]), int(bgr.shape[0])


def privacy_mask_batch(tensors, masks_per_tensor):
    """Privacy masks (csrc/vep/mask.h; the dicts of :mod:`..privacy`) applied IN PLACE to a list of
    contiguous ``[H, W, 3]`` BGR24 device tensors of any sizes on one device, each with its own
    list (an empty list leaves its picture alone): one kernel launch per level for all pictures,
    so one launch when no two masks of a picture overlap. Returns the tensors. Byte-identical with
    :func:`privacy_mask_reference`. No CPU fallback."""
    from .. import privacy

    tensors = list(tensors)
    masks_per_tensor = list(masks_per_tensor)
    if len(tensors) != len(masks_per_tensor):
        raise ValueError("masks_per_tensor must hold one list per tensor")
    device, work = None, []
    for k, (bgr, masks) in enumerate(zip(tensors, masks_per_tensor)):
        w, h = _check_mask_picture(bgr, f"tensors[{k}]")
        if not bgr.is_cuda:
            raise ValueError("bgr must be a device tensor")
        if device is None:
            device = bgr.device
        if bgr.device != device:
            raise ValueError("the pictures must live on one device")
        work.append((bgr.data_ptr(), w, h, privacy.to_native(masks)))
    require_gpu()
    if work and any(wk[3] for wk in work):
        with torch.cuda.device(device):
            native.mask_apply(work, int(torch.cuda.current_stream(device).cuda_stream))
    return tensors


def privacy_mask(bgr: torch.Tensor, masks):
    """The privacy masks of ``masks`` applied in list order, IN PLACE, to a contiguous ``[H, W, 3]``
    BGR24 device tensor, which is returned. ``fill`` sets a rect to a colour; ``pixelate`` replaces
    every ``block x block`` block of the rect (anchored at its corner, edge blocks partial) by its
    rounded mean, in integers. Bytes outside the rects are not written."""
    return privacy_mask_batch([bgr], [masks])[0]


def privacy_mask_reference(bgr: torch.Tensor, masks) -> torch.Tensor:
    """The CPU implementation's result for the same picture (host or device tensor): a new host
    tensor, the byte-exact oracle of :func:`privacy_mask`."""
    from .. import privacy

    _check_mask_picture(bgr)
    out = bgr.detach().cpu().clone().numpy()
    native.mask_apply_cpu(out, privacy.to_native(masks))
    return torch.from_numpy(out)


def _check_crop_args(width, height, fit, pad):
    from .. import crops

    width, height = crops.size(width, height)
    return width, height, crops.fit_index(fit), crops.pad_tuple(pad)


def crop_resize_batch(pictures, boxes_per_picture, width: int, height: int, fit: str = "stretch",
                      pad=(114, 114, 114), out: torch.Tensor | None = None) -> torch.Tensor:
    """The boxes (dicts ``{"x0", "y0", "x1", "y1"}`` in 1/10000 of the picture, :mod:`..crops`) of
    a list of contiguous ``[H, W, 3]`` BGR24 device tensors of any sizes on one device, each with
    its own list of at most 64 boxes, cut and resized to ``[n, height, width, 3]`` (``n`` the boxes
    of all pictures, in list order) in ONE kernel launch. A box reduces by area averaging and
    enlarges bilinearly (half-pixel centres, clamped edges), each axis on its own, exact in
    integers; ``fit="letterbox"`` keeps the aspect and fills the rest with ``pad`` ``(b, g, r)``.
    ``out``: a contiguous uint8 tensor of that shape on the pictures' device (a view at any byte
    offset will do). Byte-identical with :func:`crop_resize_reference`. No CPU fallback."""
    from .. import crops

    pictures = list(pictures)
    boxes_per_picture = list(boxes_per_picture)
    if len(pictures) != len(boxes_per_picture):
        raise ValueError("boxes_per_picture must hold one list per picture")
    width, height, fit, pad = _check_crop_args(width, height, fit, pad)
    device, work, n = None, [], 0
    for k, (bgr, boxes) in enumerate(zip(pictures, boxes_per_picture)):
        if not isinstance(bgr, torch.Tensor):
            raise TypeError(f"pictures[{k}] must be a tensor")
        w, h = _check_bgr(bgr, f"pictures[{k}]")
        if not bgr.is_cuda:
            raise ValueError("bgr must be a device tensor")
        if device is None:
            device = bgr.device
        if bgr.device != device:
            raise ValueError("the pictures must live on one device")
        work.append((bgr.data_ptr(), w, h, crops.to_native(boxes)))
        n += len(work[-1][3])
    if device is None:
        if out is None:
            raise ValueError("pictures must hold at least one picture")
        device = out.device
    require_gpu()
    shape = (n, height, width, 3)
    if out is None:
        out = torch.empty(shape, dtype=torch.uint8, device=device)
    if not (isinstance(out, torch.Tensor) and out.is_cuda and out.device == device and out.dtype == torch.uint8
            and out.is_contiguous() and tuple(out.shape) == shape):
        raise ValueError(f"out must be a contiguous uint8 tensor of shape {shape} on the pictures' device")
    if n:
        with torch.cuda.device(device):
            native.crop_resize(work, width, height, fit, pad, out.data_ptr(), out.numel(),
                               int(torch.cuda.current_stream(device).cuda_stream))
    return out


def crop_resize(bgr: torch.Tensor, boxes, width: int, height: int, fit: str = "stretch", pad=(114, 114, 114),
                out: torch.Tensor | None = None) -> torch.Tensor:
    """The boxes of one ``[H, W, 3]`` BGR24 device tensor as ``[n, height, width, 3]``: see
    :func:`crop_resize_batch`."""
    return crop_resize_batch([bgr], [boxes], width, height, fit, pad, out)


def crop_resize_reference(bgr: torch.Tensor, boxes, width: int, height: int, fit: str = "stretch",
                          pad=(114, 114, 114)) -> torch.Tensor:
    """The CPU implementation's result for the same picture (host or device tensor), on the host:
    the byte-exact oracle of :func:`crop_resize`."""
    from .. import crops

    if not isinstance(bgr, torch.Tensor):
        raise TypeError("bgr must be a tensor")
    _check_bgr(bgr)
    width, height, fit, pad = _check_crop_args(width, height, fit, pad)
    return torch.from_numpy(native.crop_resize_cpu(bgr.detach().cpu().numpy(), crops.to_native(boxes), width, height,
                                                   fit, pad))


def _check_overlay_picture(bgr, what: str) -> tuple:
    """``(width, height, pitch)`` of a ``[H, W, 3]`` uint8 tensor whose rows are packed BGR24 at
    any byte offset and any pitch ``>= 3 W`` (a contiguous tensor, or a strided view of a buffer)."""
    if not isinstance(bgr, torch.Tensor):
        raise TypeError(f"{what} must be a tensor")
    if bgr.dtype != torch.uint8:
        raise TypeError(f"{what} must be uint8")
    if bgr.dim() != 3 or bgr.shape[2] != 3 or bgr.shape[0] < 1 or bgr.shape[1] < 1:
        raise ValueError(f"{what} must be [H, W, 3], got {tuple(bgr.shape)}")
    h, w = int(bgr.shape[0]), int(bgr.shape[1])
    if h > 65535 or w > 65535:
        raise ValueError(f"{what} is at most 65535 x 65535")
    pitch = int(bgr.stride(0)) if h > 1 else w * 3
    if bgr.stride(2) != 1 or (w > 1 and bgr.stride(1) != 3) or pitch < w * 3:
        raise ValueError(f"{what} must have packed rows: strides (pitch >= 3 W, 3, 1)")
    return w, h, pitch


def _overlay_span(t: torch.Tensor, w: int, h: int, pitch: int) -> tuple:
    return t.data_ptr(), t.data_ptr() + (h - 1) * pitch + w * 3


def overlay_draw_batch(pictures, items_per_picture, outs=None, name: str = "", meta=None):
    """On-screen display (csrc/vep/overlay.h; the dicts of :mod:`..overlay`) drawn onto a list of
    ``[H, W, 3]`` BGR24 device tensors of any sizes on one device, each with its own list of at most
    64 items, in ONE kernel launch. A picture's rows may start at any byte address and have any
    pitch (a strided view will do). ``outs`` None: IN PLACE; else one tensor (or None: in place) per
    picture of the same size, which receives the picture with the items drawn on while the picture
    itself stays as it is; a picture and its output must not overlap. ``name`` and ``meta``
    (``{"seq", "timestamp"}``) replace ``{name}``, ``{seq}`` and ``{time}``. Returns the tensors
    drawn on. Byte-identical with :func:`overlay_draw_reference`. No CPU fallback."""
    from .. import overlay

    pictures = list(pictures)
    items_per_picture = list(items_per_picture)
    if len(pictures) != len(items_per_picture):
        raise ValueError("items_per_picture must hold one list per picture")
    outs = [None] * len(pictures) if outs is None else list(outs)
    if len(outs) != len(pictures):
        raise ValueError("outs must hold one entry per picture")
    if not isinstance(name, str):
        raise TypeError("name must be a string")
    if meta is not None and not isinstance(meta, dict):
        raise TypeError("meta must be a dict or None")
    device, work, res, spans = None, [], [], []
    for k, (bgr, items, out) in enumerate(zip(pictures, items_per_picture, outs)):
        w, h, pitch = _check_overlay_picture(bgr, f"pictures[{k}]")
        if not bgr.is_cuda:
            raise ValueError("bgr must be a device tensor")
        if device is None:
            device = bgr.device
        if bgr.device != device:
            raise ValueError("the pictures must live on one device")
        dst, dpitch = bgr, pitch
        if out is not None:
            ow, oh, dpitch = _check_overlay_picture(out, f"outs[{k}]")
            if (ow, oh) != (w, h) or not out.is_cuda or out.device != device:
                raise ValueError(f"outs[{k}] must be a [{h}, {w}, 3] tensor on the picture's device")
            dst = out
            a, b = _overlay_span(bgr, w, h, pitch), _overlay_span(out, w, h, dpitch)
            if a[0] < b[1] and b[0] < a[1]:
                raise ValueError(f"pictures[{k}] and outs[{k}] overlap")
        for s in spans:
            d = _overlay_span(dst, w, h, dpitch)
            if d[0] < s[1] and s[0] < d[1]:
                raise ValueError("the destinations of one call must not overlap")
        spans.append(_overlay_span(dst, w, h, dpitch))
        work.append((bgr.data_ptr(), pitch, dst.data_ptr(), dpitch, w, h, overlay.to_native(items)))
        res.append(dst)
    if work:
        require_gpu()
        with torch.cuda.device(device):
            native.overlay_draw(work, name, meta, int(torch.cuda.current_stream(device).cuda_stream))
    return res


def overlay_draw(bgr: torch.Tensor, items, out: torch.Tensor | None = None, name: str = "", meta=None) -> torch.Tensor:
    """The items drawn onto one ``[H, W, 3]`` BGR24 device tensor, in place when ``out`` is None:
    see :func:`overlay_draw_batch`. Returns the tensor drawn on."""
    return overlay_draw_batch([bgr], [items], None if out is None else [out], name, meta)[0]


def overlay_draw_reference(bgr: torch.Tensor, items, name: str = "", meta=None) -> torch.Tensor:
    """The CPU implementation's result for the same picture (host or device tensor): a new host
    tensor, the byte-exact oracle of :func:`overlay_draw`."""
    from .. import overlay

    _check_overlay_picture(bgr, "bgr")
    src = bgr.detach().cpu().contiguous().numpy()
    out = src.copy()
    native.overlay_draw_cpu(src, out, overlay.to_native(items), name, meta)
    return torch.from_numpy(out)


# ----------------------------------------------------------------------------- references

def nv12_to_bgr_reference(y: torch.Tensor, uv: torch.Tensor, width=None, height=None,
                          crop_left=0, crop_top=0) -> torch.Tensor:
    """Bit-exact oracle of the conversion kernel's integer arithmetic (BT.601 limited range,
    nearest chroma): each channel = floor((c + k*d + 2^15) / 2^16) with the kernel's 16.16
    coefficients. It shares the kernel's constants, so it pins the implementation, not the colour
    science: ``nv12_to_bgr_bt601_float`` is the independent check (±1 LSB)."""
    H, W = y.shape
    width = W - crop_left if width is None else width
    height = H - crop_top if height is None else height
    Y = y[crop_top:crop_top + height, crop_left:crop_left + width].to(torch.int64)
    xs = torch.arange(crop_left, crop_left + width, device=y.device) // 2 * 2
    ys = torch.arange(crop_top, crop_top + height, device=y.device) // 2
    U = uv[ys][:, xs].to(torch.int64)
    V = uv[ys][:, xs + 1].to(torch.int64)
    c = (Y - 16) * 76309 + 32768
    d, e = U - 128, V - 128
    r = torch.div(c + 104597 * e, 65536, rounding_mode="floor")
    g = torch.div(c - 25675 * d - 53279 * e, 65536, rounding_mode="floor")
    b = torch.div(c + 132201 * d, 65536, rounding_mode="floor")
    return torch.stack([b, g, r], dim=-1).clamp(0, 255).to(torch.uint8)


def nv12_to_bgr_bt601_float(y: torch.Tensor, uv: torch.Tensor, width=None, height=None,
                            crop_left=0, crop_top=0) -> torch.Tensor:
    """Independent float64 BT.601 limited-range YCbCr -> BGR (what swscale's default converts,
    read_image.py:94 ``to_ndarray('bgr24')``), derived from the standard's definitions rather than
    from any fixed-point constants: Kr = 0.299, Kb = 0.114, luma scaled by 255/219 from
    [16, 235], chroma by 255/224 around 128; round to nearest, clip to [0, 255]. Nearest chroma
    sample (4:2:0, the sample at or left of / above the luma position)."""
    H, W = y.shape
    width = W - crop_left if width is None else width
    height = H - crop_top if height is None else height
    kr, kb = 0.299, 0.114
    kg = 1.0 - kr - kb
    Y = (y[crop_top:crop_top + height, crop_left:crop_left + width].to(torch.float64) - 16.0) * (255.0 / 219.0)
    xs = torch.arange(crop_left, crop_left + width, device=y.device) // 2 * 2
    ys = torch.arange(crop_top, crop_top + height, device=y.device) // 2
    pb = (uv[ys][:, xs].to(torch.float64) - 128.0) * (255.0 / 224.0)
    pr = (uv[ys][:, xs + 1].to(torch.float64) - 128.0) * (255.0 / 224.0)
    r = Y + 2.0 * (1.0 - kr) * pr
    b = Y + 2.0 * (1.0 - kb) * pb
    g = Y - (2.0 * (1.0 - kb) * kb / kg) * pb - (2.0 * (1.0 - kr) * kr / kg) * pr
    bgr = torch.stack([b, g, r], dim=-1)
    return torch.floor(bgr + 0.5).clamp(0, 255).to(torch.uint8)


def letterbox_reference(bgr: torch.Tensor, size: int = 640, pad_value: int = 114,
                        chw_dtype=None, mean=(0.0, 0.0, 0.0), std=(1.0, 1.0, 1.0)):
    """fp32 torch reference: bilinear (align_corners=False) resize + centred pad."""
    import torch.nn.functional as F

    h, w = bgr.shape[:2]
    nw, nh, px, py = letterbox_geometry(w, h, size)
    x = bgr.permute(2, 0, 1)[None].float()
    r = F.interpolate(x, size=(nh, nw), mode="bilinear", align_corners=False, antialias=False)[0]
    canvas = torch.full((3, size, size), float(pad_value), device=bgr.device)
    canvas[:, py:py + nh, px:px + nw] = r
    hwc = (canvas + 0.5).clamp(0, 255).floor().to(torch.uint8).permute(1, 2, 0).contiguous()
    chw = None
    if chw_dtype is not None:
        rgb = canvas.flip(0) / 255.0
        m = torch.tensor(mean, device=bgr.device).view(3, 1, 1)
        s = torch.tensor(std, device=bgr.device).view(3, 1, 1)
        chw = ((rgb - m) / s).to(chw_dtype)
    return hwc, chw
