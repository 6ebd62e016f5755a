// The serving reads: the Worker methods that answer a client from a camera's ring (frames, scaled
// enhanced and denoised frames, JPEGs, the wall, history, motion, tamper and crops), the serve-buffer pool they copy
// through, and the VideoFrame wire encoding. Every read follows the consistent-read rule of
// ring_read.h.
#include <algorithm>
#include <cstring>

#include "clahe.h"
#include "crop.h"
#include "dehaze.h"
#include "deinterlace.h"
#include "denoise.h"
#include "dewarp.h"
#include "jpeg.h"
#include "orient.h"
#include "ring_read.h"
#include "runtime.h"
#include "scale.h"

namespace vep {

bool Worker::read_latest(int cam, i64 after, FrameMeta* meta, u8* dst, size_t cap) {
  std::shared_ptr<Camera> c = camera(cam);
  if (!c) return false;
  std::shared_ptr<FrameRing> r = c->ring();
  return r && read_latest(*r, after, meta, dst, cap);
}

void Worker::set_wall_max_tiles(int n) {
  VEP_CHECK(n >= 1 && n <= 65535, "wall: wall_max_tiles must be 1..65535");
  wall_max_tiles_.store(n);
}

void Worker::encode_device(const u8* d_bgr, int w, int h, int quality, std::string& out) {
  if (jpeg_pool_.encode(d_bgr, w, h, quality, serve_stream_, out)) return;
  // the kernels reported an overflow of their scratch: encode the picture on the host
  const size_t n = size_t(w) * size_t(h) * 3;
  std::unique_ptr<u8[]> host(new u8[n]);
  VEP_HIP(hipMemcpyAsync(host.get(), d_bgr, n, hipMemcpyDeviceToHost, serve_stream_));
  VEP_HIP(hipStreamSynchronize(serve_stream_));
  out = jpeg::encode_cpu(host.get(), w, h, quality);
}

void Worker::scale_slot(gpu::ScaleSet& set, const FrameRing& ring, int slot, int ow, int oh) {
  scale_picture(set, ring.slot_ptr(slot), ring.width(), ring.height(), ow, oh);
}

void Worker::scale_picture(gpu::ScaleSet& set, const u8* src, int sw, int sh, int ow, int oh) {
  gpu::ScaleDesc& d = set.h_descs.p[0];
  d = gpu::ScaleDesc{};
  d.src = src;
  d.sw = sw;
  d.sh = sh;
  d.src_pitch = u32(sw) * 3;
  d.dst = set.canvas.p;
  d.dst_pitch = u32(ow) * 3;
  d.ow = ow;
  d.oh = oh;
  gpu::check_scale(d, ow, oh);
  set.run(1, serve_stream_);
}

// Enhancement of the picture that is served (clahe.h, docs/ENHANCE.md): the three launches on the
// serving stream, behind the scale and ahead of the overlay and the encoder; in place when dst is
// src. The caller holds the set until it has waited for the stream.
void Worker::enhance_device(gpu::ClaheSet& set, const u8* src, size_t src_bytes, u8* dst, size_t dst_bytes, int w, int h,
                            const clahe::Params& p) {
  size_t tile_at = 0;
  set.put(0, src, src_bytes, u32(w) * 3, dst, dst_bytes, u32(w) * 3, w, h, p, tile_at);
  set.run(1, serve_stream_);
}

// The newest frame with seq > after, fitted into width x height: consume(set, host, f) gets the
// f.w x f.h picture, on a GPU in set->canvas (scaled on the serving stream, not waited for; the
// set has `download` times its bytes of pinned room), on the CPU backend in `host` (set null).
// enhance (non-null): the scaled picture is enhanced in place before consume sees it.
template <class Consume>
bool Worker::read_scaled(int cam, i64 after, int width, int height, bool download, FrameMeta* meta,
                         const clahe::Params* enhance, Consume&& consume) {
  if (enhance) clahe::check_params(*enhance);
  VEP_CHECK(width >= 0 && width <= scale::kMaxSide && height >= 0 && height <= scale::kMaxSide && (width || height),
            "scale: width and height must be 1..65535");
  std::shared_ptr<Camera> c = camera(cam);
  if (!c) return false;
  std::shared_ptr<FrameRing> ring = c->ring();
  if (!ring) return false;
  const scale::Size f = scale::fit(ring->width(), ring->height(), width, height);
  const size_t n = size_t(f.w) * size_t(f.h) * 3;
  const bool ok = read_consistent(*ring, after, meta, [&](int slot, const FrameMeta&) {
    std::vector<u8> host;
    if (dev_.gpu()) {
      dev_.bind();
      gpu::ScalePool::Lease set = scale_pool_.acquire();
      set->reserve(n, 1, download ? n : 0);
      scale_slot(*set, *ring, slot, f.w, f.h);
      gpu::ClahePool::Lease eq;  // (after the scale's set; held until consume has waited for the stream)
      if (enhance) {
        eq = clahe_pool_.acquire();
        eq->reserve(1, gpu::clahe_tiles(f.w, f.h, enhance->tile), 0, 0);
        enhance_device(*eq, set->canvas.p, n, set->canvas.p, n, f.w, f.h, *enhance);
      }
      consume(set.get(), host, f);
    } else {
      host.resize(n);
      scale::area_cpu(ring->slot_ptr(slot), ring->width(), ring->height(), size_t(ring->width()) * 3, host.data(),
                      size_t(f.w) * 3, f.w, f.h);
      if (enhance) clahe::enhance_cpu(host.data(), size_t(f.w) * 3, host.data(), size_t(f.w) * 3, f.w, f.h, *enhance);
      consume(nullptr, host, f);
    }
  });
  if (ok) {
    meta->width = f.w;
    meta->height = f.h;
    if (enhance) enhance_requests_ += 1;
  }
  return ok;
}

bool Worker::read_latest_scaled(int cam, i64 after, int width, int height, FrameMeta* meta, std::vector<u8>& dst,
                                const clahe::Params* enhance, const denoise::Params* denoise, int* denoise_frames,
                                const dehaze::Params* dehaze, u32* air) {
  if (denoise || dehaze) {
    DenoisedRead rq;
    rq.dn = denoise;
    rq.width = width;
    rq.height = height;
    rq.dehaze = dehaze;
    rq.air = air;
    rq.enhance = enhance;
    return read_denoised(cam, after, rq, meta, denoise_frames, nullptr, &dst);
  }
  return read_scaled(cam, after, width, height, true, meta, enhance, [&](gpu::ScaleSet* set, std::vector<u8>& host, scale::Size f) {
    if (!set) {
      dst.swap(host);
      return;
    }
    const size_t n = size_t(f.w) * size_t(f.h) * 3;
    VEP_HIP(hipMemcpyAsync(set->upload.p, set->canvas.p, n, hipMemcpyDeviceToHost, serve_stream_));
    VEP_HIP(hipEventRecord(set->ev, serve_stream_));
    VEP_HIP(hipEventSynchronize(set->ev));
    dst.assign(set->upload.p, set->upload.p + n);
  });
}

void Worker::read_wall_jpeg(const std::vector<int>& cams, int cols, int tw, int th, int quality,
                            const std::vector<ForeignTile>& foreign, std::vector<i64>& seqs_out, std::string& out) {
  wall_jpeg(cams, cols, tw, th, quality, foreign, nullptr, seqs_out, out);
}

void Worker::read_wall_jpeg_labelled(const std::vector<int>& cams, int cols, int tw, int th, int quality,
                                     const std::vector<ForeignTile>& foreign, const std::vector<std::string>& labels,
                                     std::vector<i64>& seqs_out, std::string& out) {
  VEP_CHECK(labels.size() == cams.size(), "wall: one label per tile expected");
  size_t labelled = 0;
  for (const std::string& l : labels) {
    VEP_CHECK(l.size() <= size_t(overlay::kMaxRawText), "overlay: a text has at most 256 bytes");
    labelled += !l.empty();
  }
  VEP_CHECK(labelled * 2 <= size_t(overlay::kMaxPrims), "overlay: the wall's labels expand to more than 256 primitives");
  wall_jpeg(cams, cols, tw, th, quality, foreign, &labels, seqs_out, out);
}

// The primitives of the wall's labels on the composed canvas: tile t's label is a text item at
// (0, 0) of its tw x th cell, expanded there (so it is clipped to the cell) and moved to the cell.
static overlay::Expanded wall_labels(const std::vector<std::string>& labels, const std::vector<char>& shown, int cols,
                                     int tw, int th) {
  overlay::Expanded all;
  for (size_t t = 0; t < labels.size(); ++t) {
    if (labels[t].empty() || !shown[t]) continue;
    overlay::Item it;
    it.kind = overlay::kTextItem;
    it.x0 = it.y0 = 0;
    it.b = it.g = it.r = 255;
    it.has_bg = 1;
    it.bg_alpha = 160;
    it.text = labels[t];
    overlay::Meta none;
    const overlay::Expanded e = overlay::expand(&it, 1, tw, th, std::string(), none);
    const int cx = int(t % size_t(cols)) * tw, cy = int(t / size_t(cols)) * th;
    for (overlay::Prim p : e.prims) {
      p.x0 = uint16_t(p.x0 + cx), p.x1 = uint16_t(p.x1 + cx), p.y0 = uint16_t(p.y0 + cy), p.y1 = uint16_t(p.y1 + cy);
      p.off = uint16_t(p.off + all.text.size());
      all.prims.push_back(p);
    }
    all.text += e.text;
  }
  VEP_CHECK(all.prims.size() <= size_t(overlay::kMaxPrims), "overlay: the wall's labels expand to more than 256 primitives");
  return all;
}

void Worker::wall_jpeg(const std::vector<int>& cams, int cols, int tw, int th, int quality,
                       const std::vector<ForeignTile>& foreign, const std::vector<std::string>* labels,
                       std::vector<i64>& seqs_out, std::string& out) {
  VEP_CHECK(quality >= 1 && quality <= 100, "jpeg: quality must be 1..100");
  const int n = int(cams.size());
  VEP_CHECK(n >= 1 && n <= wall_max_tiles(), "wall: the number of tiles must be 1..serving.wall_max_tiles");
  VEP_CHECK(tw >= 1 && tw <= scale::kMaxSide && th >= 1 && th <= scale::kMaxSide, "wall: tile size must be 1..65535");
  VEP_CHECK(cols >= 0 && cols <= scale::kMaxSide, "wall: cols out of range");
  VEP_CHECK(foreign.empty() || int(foreign.size()) == n, "wall: one foreign tile entry per tile expected");
  const scale::Wall g = scale::wall(n, cols, tw, th);
  VEP_CHECK(i64(g.cols) * tw <= scale::kMaxSide && i64(g.rows) * th <= scale::kMaxSide,
            "wall: canvas sides must be <= 65535");
  struct TileSrc {
    std::shared_ptr<Camera> cam;
    std::shared_ptr<FrameRing> ring;
    FrameMeta meta;
    int slot = -1;
    bool done = false;  // consistent, foreign or given up (background)
  };
  std::vector<TileSrc> ts((size_t(n)));
  seqs_out.assign(size_t(n), 0);
  size_t up_bytes = 0;
  for (int t = 0; t < n; ++t) {
    TileSrc& s = ts[size_t(t)];
    if (!foreign.empty() && foreign[size_t(t)].data) {
      const ForeignTile& f = foreign[size_t(t)];
      VEP_CHECK(f.w >= 1 && f.h >= 1 && f.w <= tw && f.h <= th, "wall: foreign tile larger than its cell");
      up_bytes += size_t(f.w) * size_t(f.h) * 3;
      seqs_out[size_t(t)] = f.seq;
      continue;
    }
    s.cam = camera(cams[size_t(t)]);
    if (s.cam) s.ring = s.cam->ring();
  }
  const size_t pitch = size_t(g.w) * 3, canvas_bytes = pitch * size_t(g.h);
  // tile t's descriptor from its ring's newest frame; background only when there is none
  auto cell = [&](int t, u8* canvas) {
    gpu::ScaleDesc d{};
    d.dst = canvas;
    d.dst_pitch = u32(pitch);
    d.cx = (t % g.cols) * tw;
    d.cy = (t / g.cols) * th;
    d.cw = tw;
    d.ch = th;
    return d;
  };
  auto pick = [&](int t) {  // newest frame of tile t's ring -> slot / meta; false: background
    TileSrc& s = ts[size_t(t)];
    s.slot = -1;
    return s.ring && s.ring->latest(0, &s.meta, &s.slot);
  };
  auto shown = [&] {  // the tiles that show a frame, once the rounds are over
    std::vector<char> v(size_t(n), 0);
    for (int t = 0; t < n; ++t) v[size_t(t)] = seqs_out[size_t(t)] != 0 || (!foreign.empty() && foreign[size_t(t)].data);
    return v;
  };
  if (!dev_.gpu()) {
    std::vector<u8> canvas(canvas_bytes);
    std::vector<scale::Tile> tiles((size_t(n)));
    for (int round = 0; round < kReadAttempts; ++round) {
      bool again = false;
      for (int t = 0; t < n; ++t) {
        TileSrc& s = ts[size_t(t)];
        scale::Tile& tl = tiles[size_t(t)];
        if (s.done && round) continue;
        tl = scale::Tile{};
        if (!foreign.empty() && foreign[size_t(t)].data) {
          s.done = true;
          continue;
        }
        if (!pick(t)) {
          s.done = true;
          continue;
        }
        tl.src = s.ring->slot_ptr(s.slot);
        tl.sw = s.ring->width();
        tl.sh = s.ring->height();
        tl.pitch = size_t(tl.sw) * 3;
      }
      // (the host composition is cheap to repeat whole: a round redraws every tile)
      scale::compose_cpu(tiles.data(), n, g.cols, tw, th, canvas.data(), pitch);
      for (int t = 0; t < n; ++t) {
        TileSrc& s = ts[size_t(t)];
        if (!tiles[size_t(t)].src) continue;
        if (s.ring->still_valid(s.slot, s.meta.seq)) {
          s.done = true;
          seqs_out[size_t(t)] = s.meta.seq;
        } else {
          s.done = false;
          seqs_out[size_t(t)] = 0;
          again = true;
        }
      }
      if (!again) break;
      if (round == kReadAttempts - 1) {  // still inconsistent: those tiles are drawn as background
        // (only their cells are cleared: the other tiles were checked after they were drawn)
        for (int t = 0; t < n; ++t) {
          if (ts[size_t(t)].done) continue;
          u8* p = canvas.data() + size_t((t / g.cols) * th) * pitch + size_t((t % g.cols) * tw) * 3;
          for (int y = 0; y < th; ++y) std::memset(p + size_t(y) * pitch, scale::kBackground, size_t(tw) * 3);
        }
      }
    }
    for (int t = 0; t < n && !foreign.empty(); ++t) {
      const ForeignTile& f = foreign[size_t(t)];
      if (!f.data) continue;
      u8* p = canvas.data() + size_t((t / g.cols) * th + (th - f.h) / 2) * pitch +
              size_t((t % g.cols) * tw + (tw - f.w) / 2) * 3;
      for (int y = 0; y < f.h; ++y) std::memcpy(p + size_t(y) * pitch, f.data + size_t(y) * f.w * 3, size_t(f.w) * 3);
    }
    if (labels) {
      const overlay::Expanded e = wall_labels(*labels, shown(), g.cols, tw, th);
      overlay_requests_ += 1;
      overlay_prims_ += e.prims.size();
      overlay::apply_cpu(canvas.data(), pitch, canvas.data(), pitch, g.w, g.h, e.prims.data(), int(e.prims.size()),
                         reinterpret_cast<const u8*>(e.text.data()), e.text.size());
    }
    out = jpeg::encode_cpu(canvas.data(), g.w, g.h, quality);
    return;
  }
  dev_.bind();
  const int cells = g.cols * g.rows;  // (the cells past the last tile are background too)
  gpu::ScalePool::Lease set = scale_pool_.acquire();
  set->reserve(canvas_bytes, cells, up_bytes);
  std::vector<int> tile_of;  // descriptor -> tile of the current round
  for (int round = 0; round <= kReadAttempts; ++round) {
    // the kReadAttempts rounds scale the tiles that are not settled; one more only clears what is left
    tile_of.clear();
    for (int t = 0; t < n; ++t) {
      TileSrc& s = ts[size_t(t)];
      if (s.done) continue;
      gpu::ScaleDesc d = cell(t, set->canvas.p);
      const bool fgn = !foreign.empty() && foreign[size_t(t)].data;
      if (!fgn && round < kReadAttempts && pick(t)) {
        const scale::Placement p = scale::place(t, g.cols, tw, th, s.ring->width(), s.ring->height());
        d.src = s.ring->slot_ptr(s.slot);
        d.sw = s.ring->width();
        d.sh = s.ring->height();
        d.src_pitch = u32(d.sw) * 3;
        d.dx = p.x;
        d.dy = p.y;
        d.ow = p.w;
        d.oh = p.h;
      } else {
        s.slot = -1;
      }
      gpu::check_scale(d, g.w, g.h);
      set->h_descs.p[tile_of.size()] = d;
      tile_of.push_back(t);
    }
    if (tile_of.empty()) break;
    int nd = int(tile_of.size());
    for (int t = n; t < cells && round == 0; ++t) {
      set->h_descs.p[nd] = cell(t, set->canvas.p);
      gpu::check_scale(set->h_descs.p[nd++], g.w, g.h);
    }
    set->run(nd, serve_stream_);
    if (round == 0 && up_bytes) {  // foreign tiles: over their (background) cells, after the launch
      size_t off = 0;
      for (int t = 0; t < n; ++t) {
        const ForeignTile& f = foreign[size_t(t)];
        if (!f.data) continue;
        const size_t row = size_t(f.w) * 3, bytes = row * size_t(f.h);
        std::memcpy(set->upload.p + off, f.data, bytes);
        u8* p = set->canvas.p + size_t((t / g.cols) * th + (th - f.h) / 2) * pitch +
                size_t((t % g.cols) * tw + (tw - f.w) / 2) * 3;
        VEP_HIP(hipMemcpy2DAsync(p, pitch, set->upload.p + off, row, row, size_t(f.h), hipMemcpyHostToDevice,
                                 serve_stream_));
        off += bytes;
      }
      VEP_HIP(hipEventRecord(set->ev, serve_stream_));  // (again: after the uploads)
    }
    VEP_HIP(hipEventSynchronize(set->ev));
    for (int t : tile_of) {
      TileSrc& s = ts[size_t(t)];
      if (s.slot < 0) {
        s.done = true;  // background or foreign
      } else if (s.ring->still_valid(s.slot, s.meta.seq)) {
        s.done = true;
        seqs_out[size_t(t)] = s.meta.seq;
      }
    }
  }
  gpu::OverlayPool::Lease osd;  // (held until the encode has waited for the stream)
  if (labels) {
    const overlay::Expanded e = wall_labels(*labels, shown(), g.cols, tw, th);
    overlay_requests_ += 1;
    overlay_prims_ += e.prims.size();
    if (!e.prims.empty()) {
      osd = overlay_pool_.acquire();
      osd->reserve(1, e.prims.size(), e.text.size(), 0);
      size_t prim_at = 0, text_at = 0;
      osd->put(0, set->canvas.p, canvas_bytes, u32(pitch), set->canvas.p, canvas_bytes, u32(pitch), g.w, g.h, e, prim_at,
               text_at);
      osd->run(1, prim_at, text_at, serve_stream_);
    }
  }
  encode_device(set->canvas.p, g.w, g.h, quality, out);
}

bool Worker::read_latest_enhanced(int cam, i64 after, int width, int height, const clahe::Params& p, FrameMeta* meta,
                                  std::vector<u8>& dst) {
  if (width || height) return read_latest_scaled(cam, after, width, height, meta, dst, &p);
  clahe::check_params(p);
  std::shared_ptr<Camera> c = camera(cam);
  if (!c) return false;
  std::shared_ptr<FrameRing> ring = c->ring();
  if (!ring) return false;
  const int w = ring->width(), h = ring->height();
  const size_t n = ring->slot_bytes();
  const bool ok = read_consistent(*ring, after, meta, [&](int slot, const FrameMeta&) {
    dst.resize(n);
    if (!dev_.gpu()) {
      clahe::enhance_cpu(ring->slot_ptr(slot), size_t(w) * 3, dst.data(), size_t(w) * 3, w, h, p);
      return;
    }
    dev_.bind();
    gpu::ClahePool::Lease eq = clahe_pool_.acquire();
    eq->reserve(1, gpu::clahe_tiles(w, h, p.tile), n, n);
    enhance_device(*eq, ring->slot_ptr(slot), n, eq->picture.p, n, w, h, p);
    VEP_HIP(hipMemcpyAsync(eq->host.p, eq->picture.p, n, hipMemcpyDeviceToHost, serve_stream_));
    VEP_HIP(hipEventRecord(eq->ev, serve_stream_));  // (again: after the copy)
    VEP_HIP(hipEventSynchronize(eq->ev));
    std::memcpy(dst.data(), eq->host.p, n);
  });
  if (ok) enhance_requests_ += 1;
  return ok;
}

// A denoised read (denoise.h, docs/DENOISE.md): the newest frames of the ring, read under the
// multi-slot rule of ring_read.h, are blended into the denoise set's picture at native size, and
// from there on that picture stands where the ring slot stands in the other reads: scaled into
// the scaler's canvas, enhanced and drawn on in place, then encoded or copied down, all on the
// serving stream. The ring's slots are only read. The CPU backend does the same on the host.
bool Worker::read_denoised(int cam, i64 after, const DenoisedRead& rq, FrameMeta* meta, int* used, std::string* jpeg,
                           std::vector<u8>* raw) {
  if (rq.dn) denoise::check_params(*rq.dn);
  if (rq.di) deinterlace::check_params(*rq.di);
  VEP_CHECK(!(rq.dn && rq.di), "deinterlace: not served together with denoise, which blends the ring's woven frames");
  VEP_CHECK(rq.orient >= 0 && rq.orient <= (orient::kT | orient::kMX | orient::kMY),
            "orient: rotate must be 0, 90, 180 or 270 and flip none, h or v");
  if (rq.dehaze) dehaze::check_params(*rq.dehaze);
  if (rq.enhance) clahe::check_params(*rq.enhance);
  VEP_CHECK(rq.width >= 0 && rq.width <= scale::kMaxSide && rq.height >= 0 && rq.height <= scale::kMaxSide,
            "scale: width and height must be 1..65535");
  if (rq.items) overlay::check_list(rq.items->data(), int(rq.items->size()));
  std::shared_ptr<Camera> c = camera(cam);
  if (!c) return false;
  std::shared_ptr<FrameRing> ring = c->ring();
  if (!ring) return false;
  VEP_CHECK(!rq.dn || ring->history() >= 2, "denoise: the camera's ring keeps no history: buffer.in_memory must be 2 or more");
  const int w = ring->width(), h = ring->height();
  // the upright picture: what the scale and every step behind it see (w x h without an orientation)
  const int uw = orient::out_w(rq.orient, w, h), uh = orient::out_h(rq.orient, w, h);
  const bool scaled = rq.width || rq.height;
  const scale::Size f = scaled ? scale::fit(uw, uh, rq.width, rq.height) : scale::Size{uw, uh};
  const size_t native = ring->slot_bytes(), n = size_t(f.w) * size_t(f.h) * 3, row = size_t(f.w) * 3;
  VEP_CHECK(!rq.dehaze || (f.w >= dehaze::kMinSide && f.h >= dehaze::kMinSide && u64(f.w) * u64(f.h) <= dehaze::kMaxPixels),
            "dehaze: both sides of the served picture must be at least 16 and the picture at most 2^24 pixels");
  size_t drawn = 0;
  int count = 0, woven = 0;
  u32 air[4] = {0, 0, 0, 0};
  VEP_CHECK(!rq.di || (w >= deinterlace::kMinSide && h >= deinterlace::kMinSide),
            "deinterlace: both sides of the picture must be 4..65535");
  // (the deinterlacer takes the frame before the newest where the ring has it, and does without)
  const int ask = rq.dn ? std::min(rq.dn->frames, ring->history()) : (rq.di && ring->history() >= 2 ? 2 : 1);
  const bool ok = read_consistent_frames(
      *ring, after, ask, meta, &count,
      [&](const std::vector<std::pair<FrameMeta, int>>& have, const FrameMeta& m) {
        deinterlace::Job dj;
        if (rq.di) {
          dj.newer = ring->slot_ptr(have[0].second);
          // the frame before: only one of the newest's size (a stream that changed its size mid-ring)
          if (have.size() > 1 && have[1].first.width == m.width && have[1].first.height == m.height)
            dj.older = ring->slot_ptr(have[1].second);
          dj.newer_bytes = dj.older_bytes = dj.dst_bytes = native;
          dj.newer_pitch = dj.older_pitch = dj.dst_pitch = u32(w) * 3;
          dj.w = dj.older_w = w;
          dj.h = dj.older_h = h;
          dj.p = *rq.di;
          woven = deinterlace::temporal_of(dj) ? 2 : 1;
        }
        denoise::Job j;
        j.frames = rq.di ? 1 : int(have.size());
        for (int k = 0; k < j.frames; ++k) {
          j.src[k] = ring->slot_ptr(have[size_t(k)].second);
          j.src_bytes[k] = native;
          j.src_pitch[k] = u32(w) * 3;
        }
        j.dst_bytes = native;
        j.dst_pitch = u32(w) * 3;
        j.w = w;
        j.h = h;
        j.level = rq.dn ? rq.dn->level : 0;
        j.strength = rq.dn ? rq.dn->strength : 0;
        orient::Job oj;  // (source and destination: below, where the step before it has its picture)
        oj.src_bytes = oj.dst_bytes = native;
        oj.src_pitch = u32(w) * 3;
        oj.dst_pitch = u32(uw) * 3;
        oj.w = w;
        oj.h = h;
        oj.op = rq.orient;
        overlay::Expanded e;  // (the items meet the picture they are drawn on, and the newest frame's meta)
        if (rq.items)
          e = overlay::expand(rq.items->data(), int(rq.items->size()), f.w, f.h, *rq.name, overlay::Meta{m.seq, m.timestamp});
        const u8* text = reinterpret_cast<const u8*>(e.text.data());
        drawn = e.prims.size();
        if (!dev_.gpu()) {
          std::vector<u8> pic(native);
          j.dst = dj.dst = pic.data();
          if (rq.dn) denoise::denoise_cpu(j);
          else if (rq.di) deinterlace::deinterlace_cpu(dj);
          else if (!rq.orient) std::memcpy(pic.data(), j.src[0], native);
          if (rq.orient) {
            std::vector<u8> upright(native);
            oj.src = rq.dn || rq.di ? pic.data() : j.src[0];
            oj.dst = upright.data();
            orient::apply_cpu(oj);
            pic.swap(upright);
          }
          if (scaled) {
            std::vector<u8> small(n);
            scale::area_cpu(pic.data(), uw, uh, size_t(uw) * 3, small.data(), row, f.w, f.h);
            pic.swap(small);
          }
          if (rq.dehaze) dehaze::dehaze_cpu(pic.data(), row, pic.data(), row, f.w, f.h, *rq.dehaze, air);
          if (rq.enhance) clahe::enhance_cpu(pic.data(), row, pic.data(), row, f.w, f.h, *rq.enhance);
          if (rq.items)
            overlay::apply_cpu(pic.data(), row, pic.data(), row, f.w, f.h, e.prims.data(), int(e.prims.size()), text,
                               e.text.size());
          if (jpeg) *jpeg = jpeg::encode_cpu(pic.data(), f.w, f.h, rq.quality);
          else raw->swap(pic);
          return;
        }
        dev_.bind();
        // (every request takes its sets in one order: denoise, deinterlace, orient, scale, dehaze, clahe, overlay, encoder)
        gpu::DenoisePool::Lease dn;
        if (rq.dn) {
          dn = denoise_pool_.acquire();
          dn->reserve(1, native, raw && !rq.dehaze ? n : 0);
        }
        gpu::DeinterlacePool::Lease di;
        if (rq.di) {
          di = deinterlace_pool_.acquire();
          di->reserve(1, native, raw && !rq.dehaze ? n : 0);
        }
        gpu::OrientPool::Lease up;
        if (rq.orient) {
          up = orient_pool_.acquire();
          up->reserve(1, native, raw && !rq.dehaze ? n : 0);
        }
        gpu::ScalePool::Lease set;
        if (scaled) {
          set = scale_pool_.acquire();
          set->reserve(n, 1, 0);
        }
        gpu::DehazePool::Lease dh;
        if (rq.dehaze) {
          dh = dehaze_pool_.acquire();
          // (a picture of its own only where the one to dehaze is the ring slot, which is never written)
          dh->reserve(1, gpu::DehazeSet::plane_words(f.w, f.h), rq.dn || rq.di || rq.orient || scaled ? 0 : n, raw ? n : 0);
        }
        gpu::ClahePool::Lease eq;
        if (rq.enhance) {
          eq = clahe_pool_.acquire();
          eq->reserve(1, gpu::clahe_tiles(f.w, f.h, rq.enhance->tile), 0, 0);
        }
        gpu::OverlayPool::Lease osd;
        if (rq.items) {
          osd = overlay_pool_.acquire();
          osd->reserve(1, e.prims.size(), e.text.size(), 0);
        }
        // (the same stream: every stage is ordered behind the one before)
        u8* pic = nullptr;  // the picture the stages work on in place; null while it is still the slot
        if (rq.dn) {
          j.dst = dn->picture.p;
          dn->put(0, j);
          dn->run(1, serve_stream_);
          pic = dn->picture.p;
        }
        if (rq.di) {
          dj.dst = di->picture.p;
          di->put(0, dj);
          di->run(1, serve_stream_);
          pic = di->picture.p;
        }
        if (rq.orient) {
          oj.src = pic ? pic : j.src[0];
          oj.dst = up->picture.p;
          up->put(0, oj);
          up->run(1, serve_stream_);
          pic = up->picture.p;
        }
        if (scaled) {
          scale_picture(*set, pic ? pic : j.src[0], uw, uh, f.w, f.h);
          pic = set->canvas.p;
        }
        if (rq.dehaze) {
          size_t plane_at = 0;
          u8* out = pic ? pic : dh->picture.p;
          const u32* d_air = dh->put(0, pic ? pic : j.src[0], n, u32(row), out, n, u32(row), f.w, f.h, *rq.dehaze, plane_at);
          dh->run(1, serve_stream_);
          // (read after the wait for the encoder or for the copy below, which this stream orders behind it)
          VEP_HIP(hipMemcpyAsync(dh->h_air.p, d_air, 4 * sizeof(u32), hipMemcpyDeviceToHost, serve_stream_));
          pic = out;
        }
        if (rq.enhance) enhance_device(*eq, pic, n, pic, n, f.w, f.h, *rq.enhance);
        if (rq.items) {
          size_t prim_at = 0, text_at = 0;
          osd->put(0, pic, n, u32(row), pic, n, u32(row), f.w, f.h, e, prim_at, text_at);
          osd->run(1, prim_at, text_at, serve_stream_);
        }
        if (jpeg) {
          encode_device(pic, f.w, f.h, rq.quality, *jpeg);
        } else {
          u8* host = rq.dehaze ? dh->host.p : (rq.orient ? up->host.p : (rq.di ? di->host.p : dn->host.p));
          hipEvent_t ev = rq.dehaze ? hipEvent_t(dh->ev)
                                    : (rq.orient ? hipEvent_t(up->ev) : (rq.di ? hipEvent_t(di->ev) : hipEvent_t(dn->ev)));
          VEP_HIP(hipMemcpyAsync(host, pic, n, hipMemcpyDeviceToHost, serve_stream_));
          VEP_HIP(hipEventRecord(ev, serve_stream_));  // (again: after the copy)
          VEP_HIP(hipEventSynchronize(ev));
          raw->assign(host, host + n);
        }
        if (rq.dehaze) std::copy_n(dh->h_air.p, 3, air);
      },
      rq.di != nullptr);
  if (!ok) return false;
  if (used) *used = rq.di ? woven : count;
  meta->width = f.w;
  meta->height = f.h;
  if (rq.dn) denoise_requests_ += 1;
  if (rq.di) deinterlace_requests_ += 1;
  if (rq.orient) orient_requests_ += 1;
  if (rq.dehaze) {
    dehaze_requests_ += 1;
    if (rq.air) std::copy_n(air, 3, rq.air);
  }
  if (rq.enhance) enhance_requests_ += 1;
  if (rq.items) {
    overlay_requests_ += 1;
    overlay_prims_ += drawn;
  }
  return true;
}

bool Worker::read_latest_denoised(int cam, i64 after, int width, int height, const denoise::Params& p, FrameMeta* meta,
                                  std::vector<u8>& dst, int* denoise_frames) {
  DenoisedRead rq;
  rq.dn = &p;
  rq.width = width;
  rq.height = height;
  return read_denoised(cam, after, rq, meta, denoise_frames, nullptr, &dst);
}

bool Worker::read_latest_deinterlaced(int cam, i64 after, int width, int height, const deinterlace::Params& p, FrameMeta* meta,
                                      std::vector<u8>& dst, int* frames) {
  DenoisedRead rq;
  rq.di = &p;
  rq.width = width;
  rq.height = height;
  return read_denoised(cam, after, rq, meta, frames, nullptr, &dst);
}

bool Worker::read_latest_oriented(int cam, i64 after, int width, int height, int op, FrameMeta* meta, std::vector<u8>& dst) {
  VEP_CHECK(op != 0, "orient: the identity is not an oriented read");
  DenoisedRead rq;
  rq.orient = op;
  rq.width = width;
  rq.height = height;
  return read_denoised(cam, after, rq, meta, nullptr, nullptr, &dst);
}

bool Worker::read_latest_dehazed(int cam, i64 after, int width, int height, const dehaze::Params& p, FrameMeta* meta,
                                 std::vector<u8>& dst, u32* air) {
  DenoisedRead rq;
  rq.dehaze = &p;
  rq.air = air;
  rq.width = width;
  rq.height = height;
  return read_denoised(cam, after, rq, meta, nullptr, nullptr, &dst);
}

bool Worker::read_latest_jpeg(int cam, i64 after, int quality, FrameMeta* meta, std::string& out, int width,
                              int height, const clahe::Params* enhance, const denoise::Params* denoise,
                              int* denoise_frames, const dehaze::Params* dehaze, u32* air,
                              const deinterlace::Params* deinterlace, int* deinterlace_frames, int orient) {
  VEP_CHECK(quality >= 1 && quality <= 100, "jpeg: quality must be 1..100");
  if (denoise || dehaze || deinterlace || orient) {
    DenoisedRead rq;
    rq.dn = denoise;
    rq.di = deinterlace;
    rq.orient = orient;
    rq.width = width;
    rq.height = height;
    rq.dehaze = dehaze;
    rq.air = air;
    rq.enhance = enhance;
    rq.quality = quality;
    return read_denoised(cam, after, rq, meta, deinterlace ? deinterlace_frames : denoise_frames, &out, nullptr);
  }
  if (width || height)
    return read_scaled(cam, after, width, height, false, meta, enhance,
                       [&](gpu::ScaleSet* set, std::vector<u8>& host, scale::Size f) {
                         // (GPU: the same stream, so the encode is ordered after the scale)
                         if (set) encode_device(set->canvas.p, f.w, f.h, quality, out);
                         else out = jpeg::encode_cpu(host.data(), f.w, f.h, quality);
                       });
  std::shared_ptr<Camera> c = camera(cam);
  if (!c) return false;
  std::shared_ptr<FrameRing> ring = c->ring();
  if (!ring) return false;
  const int w = ring->width(), h = ring->height();
  if (enhance) {  // out of place from the slot, which is never written; the encoder chained behind
    clahe::check_params(*enhance);
    const size_t n = ring->slot_bytes();
    const bool ok = read_consistent(*ring, after, meta, [&](int slot, const FrameMeta&) {
      if (!dev_.gpu()) {
        std::vector<u8> host(n);
        clahe::enhance_cpu(ring->slot_ptr(slot), size_t(w) * 3, host.data(), size_t(w) * 3, w, h, *enhance);
        out = jpeg::encode_cpu(host.data(), w, h, quality);
        return;
      }
      dev_.bind();
      gpu::ClahePool::Lease eq = clahe_pool_.acquire();
      eq->reserve(1, gpu::clahe_tiles(w, h, enhance->tile), n, 0);
      enhance_device(*eq, ring->slot_ptr(slot), n, eq->picture.p, n, w, h, *enhance);
      encode_device(eq->picture.p, w, h, quality, out);
    });
    if (ok) enhance_requests_ += 1;
    return ok;
  }
  return read_consistent(*ring, after, meta, [&](int slot, const FrameMeta&) {
    if (!dev_.gpu()) {
      out = jpeg::encode_cpu(ring->slot_ptr(slot), w, h, quality);
      return;
    }
    dev_.bind();
    if (jpeg_pool_.encode(ring->slot_ptr(slot), w, h, quality, serve_stream_, out)) return;
    // the kernels reported an overflow of their scratch: encode the frame on the host
    std::unique_ptr<u8[]> host(new u8[ring->slot_bytes()]);
    copy_slot(*ring, slot, host.get());
    out = jpeg::encode_cpu(host.get(), w, h, quality);
  });
}

bool Worker::read_overlay_jpeg(int cam, i64 after, int quality, const std::vector<overlay::Item>& items,
                               const std::string& name, FrameMeta* meta, std::string& out, int width, int height,
                               const clahe::Params* enhance, const denoise::Params* denoise, int* denoise_frames,
                               const dehaze::Params* dehaze, u32* air, const deinterlace::Params* deinterlace,
                               int* deinterlace_frames, int orient) {
  VEP_CHECK(quality >= 1 && quality <= 100, "jpeg: quality must be 1..100");
  if (denoise || dehaze || deinterlace || orient) {
    DenoisedRead rq;
    rq.dn = denoise;
    rq.di = deinterlace;
    rq.orient = orient;
    rq.width = width;
    rq.height = height;
    rq.dehaze = dehaze;
    rq.air = air;
    rq.enhance = enhance;
    rq.items = &items;
    rq.name = &name;
    rq.quality = quality;
    return read_denoised(cam, after, rq, meta, deinterlace ? deinterlace_frames : denoise_frames, &out, nullptr);
  }
  if (enhance) clahe::check_params(*enhance);
  VEP_CHECK(width >= 0 && width <= scale::kMaxSide && height >= 0 && height <= scale::kMaxSide,
            "scale: width and height must be 1..65535");
  overlay::check_list(items.data(), int(items.size()));
  std::shared_ptr<Camera> c = camera(cam);
  if (!c) return false;
  std::shared_ptr<FrameRing> ring = c->ring();
  if (!ring) return false;
  const int w = ring->width(), h = ring->height();
  const bool scaled = width || height;
  const scale::Size f = scaled ? scale::fit(w, h, width, height) : scale::Size{w, h};
  const size_t n = size_t(f.w) * size_t(f.h) * 3, row = size_t(f.w) * 3;
  size_t drawn = 0;
  const bool ok = read_consistent(*ring, after, meta, [&](int slot, const FrameMeta& m) {
    // (the items meet the picture they are drawn on, and the meta of the frame picked this time)
    const overlay::Expanded e =
        overlay::expand(items.data(), int(items.size()), f.w, f.h, name, overlay::Meta{m.seq, m.timestamp});
    const u8* text = reinterpret_cast<const u8*>(e.text.data());
    drawn = e.prims.size();
    if (!dev_.gpu()) {
      std::vector<u8> host(n);
      if (scaled || enhance) {
        if (scaled) scale::area_cpu(ring->slot_ptr(slot), w, h, size_t(w) * 3, host.data(), row, f.w, f.h);
        if (enhance) clahe::enhance_cpu(scaled ? host.data() : ring->slot_ptr(slot), row, host.data(), row, f.w, f.h, *enhance);
        overlay::apply_cpu(host.data(), row, host.data(), row, f.w, f.h, e.prims.data(), int(e.prims.size()), text,
                           e.text.size());
      } else {
        overlay::apply_cpu(ring->slot_ptr(slot), row, host.data(), row, w, h, e.prims.data(), int(e.prims.size()), text,
                           e.text.size());
      }
      out = jpeg::encode_cpu(host.data(), f.w, f.h, quality);
      return;
    }
    dev_.bind();
    // (every request takes its sets in one order: scale, clahe, overlay, encoder)
    gpu::ScalePool::Lease set;
    if (scaled) {
      set = scale_pool_.acquire();
      set->reserve(n, 1, 0);
    }
    gpu::ClahePool::Lease eq;
    if (enhance) {
      eq = clahe_pool_.acquire();
      eq->reserve(1, gpu::clahe_tiles(f.w, f.h, enhance->tile), scaled ? 0 : n, 0);
    }
    gpu::OverlayPool::Lease osd = overlay_pool_.acquire();
    osd->reserve(1, e.prims.size(), e.text.size(), scaled || enhance ? 0 : n);
    size_t prim_at = 0, text_at = 0;
    if (scaled || enhance) {
      // (the same stream: enhanced after the scale, drawn after that, encoded after the drawing)
      u8* pic = scaled ? set->canvas.p : eq->picture.p;  // the scaler's canvas, or the slot's enhanced copy
      if (scaled) scale_slot(*set, *ring, slot, f.w, f.h);
      if (enhance) enhance_device(*eq, scaled ? pic : ring->slot_ptr(slot), n, pic, n, f.w, f.h, *enhance);
      osd->put(0, pic, n, u32(row), pic, n, u32(row), f.w, f.h, e, prim_at, text_at);
      osd->run(1, prim_at, text_at, serve_stream_);
      encode_device(pic, f.w, f.h, quality, out);
    } else {
      osd->put(0, ring->slot_ptr(slot), ring->slot_bytes(), u32(row), osd->picture.p, n, u32(row), w, h, e, prim_at,
               text_at);
      osd->run(1, prim_at, text_at, serve_stream_);
      encode_device(osd->picture.p, w, h, quality, out);
    }
  });
  if (ok) {
    overlay_requests_ += 1;
    overlay_prims_ += drawn;
    if (enhance) enhance_requests_ += 1;
  }
  if (ok && scaled) {
    meta->width = f.w;
    meta->height = f.h;
  }
  return ok;
}

// ------------------------------------------------------------------------- motion detection

void Worker::motion_free(MotionState& st) {
  if (st.bg[0] || st.bg[1]) dev_.bind();
  dev_.free(st.bg[0]);
  dev_.free(st.bg[1]);
  st.bg[0] = st.bg[1] = nullptr;
  st.samples = 0;
  st.w = st.h = 0;
  st.cur = 0;
  st.have_bg = false;
  st.seq = 0;
  st.ring.reset();
  st.result = MotionResult{};
}

void Worker::set_motion_params(const motion::Params& p) {
  motion::check_params(p);
  {
    std::lock_guard<std::mutex> g(motion_mu_);
    motion_params_ = p;
    ++motion_gen_;  // a model of an older generation counts as none
  }
  std::vector<std::shared_ptr<Camera>> cams;
  {
    std::lock_guard<std::mutex> g(cams_mu_);
    cams = cams_;
  }
  for (auto& c : cams) {
    if (!c) continue;
    std::lock_guard<std::mutex> g(c->motion.mu);
    motion_free(c->motion);
  }
}

motion::Params Worker::motion_params() {
  std::lock_guard<std::mutex> g(motion_mu_);
  return motion_params_;
}

void Worker::motion_reset(int cam) {
  std::shared_ptr<Camera> c = camera(cam);
  VEP_CHECK(c, "no such camera");
  std::lock_guard<std::mutex> g(c->motion.mu);
  motion_free(c->motion);
}

// One camera of a motion or tamper request. Its state's mutex is held from pick to commit.
template <class Result, class Entry = ReadEntry>
struct CamEval : Entry {
  int cam = -1;
  std::shared_ptr<Camera> c;
  std::unique_lock<std::mutex> lock;
  Result result;
};

// The rounds of read_consistent_rounds over the cameras' states (op: Worker::MotionOp or
// TamperOp). evs: distinct cameras in ascending index (the order their mutexes are taken in).
template <class Eval, class Op>
static void eval_cameras(Worker& w, std::vector<Eval>& evs, Op& op) {
  // (every camera is looked up before the first state mutex is taken: remove_camera takes a
  // state's mutex with the camera table locked)
  for (Eval& e : evs) {
    e.c = w.camera(e.cam);
    if (e.c) e.ring = e.c->ring();
  }
  for (Eval& e : evs) {
    if (!e.ring) continue;
    e.lock = std::unique_lock<std::mutex>(Op::state(*e.c).mu);
    e.pending = Op::live(*e.c);
  }
  // (after the cameras' mutexes: set_motion_params / set_tamper_params store the parameters before
  // they take them, so a model or an answer built here under older parameters is reset by them
  // afterwards)
  op.snapshot();
  read_consistent_rounds(evs, op);
  for (Eval& e : evs)
    if (e.lock.owns_lock()) e.lock.unlock();
}

// A request's cameras, each evaluated once; and the one-camera case (out may be null).
template <class Op, class Result>
static void read_cameras(Worker& w, Op& op, const std::vector<int>& cams, i64 after, std::vector<Result>& out,
                         std::vector<char>& ok) {
  read_each_once<typename Op::Eval>(cams, after, out, ok,
                                    [&](std::vector<typename Op::Eval>& evs) { eval_cameras(w, evs, op); });
}
template <class Op, class Result>
static bool read_camera(Worker& w, Op& op, int cam, i64 after, Result* out) {
  std::vector<Result> res;
  std::vector<char> ok;
  read_cameras(w, op, {cam}, after, res, ok);
  if (ok[0] && out) *out = std::move(res[0]);
  return ok[0] != 0;
}

struct Worker::MotionOp {
  struct Eval : CamEval<MotionResult> {
    bool primed = false;       // this evaluation has a model to compare with
    size_t cells = 0, at = 0;  // its grid in the request's counts buffer
    std::vector<u32> counts;
  };
  Worker& w;
  motion::Params prm;
  u64 gen = 0;
  static MotionState& state(Camera& c) { return c.motion; }
  static bool live(Camera& c) { return !c.motion.removed; }
  void snapshot() {
    std::lock_guard<std::mutex> g(w.motion_mu_);
    prm = w.motion_params_;
    gen = w.motion_gen_;
  }
  bool stored(Eval& e) {
    MotionState& st = e.c->motion;
    const bool same_ring = st.ring.lock() == e.ring;
    if (st.gen != gen || !same_ring || st.w != e.ring->width() || st.h != e.ring->height()) {
      w.motion_free(st);  // other parameters, a new ring or a new size: prime again
      st.gen = gen;
      st.ring = e.ring;
    }
    if (st.seq != e.meta.seq || st.seq == 0) return false;
    e.result = st.result;  // evaluated already: one evaluation per frame
    return true;
  }
  void plan(Eval& e) {
    MotionState& st = e.c->motion;
    const int pw = e.ring->width(), ph = e.ring->height();
    if (!st.bg[0]) {
      const size_t samples = size_t(motion::pitch_for(u32(pw))) * size_t(ph);
      w.dev_.bind();
      st.bg[0] = static_cast<u16*>(w.dev_.alloc(samples * sizeof(u16)));
      st.bg[1] = static_cast<u16*>(w.dev_.alloc(samples * sizeof(u16)));
      st.samples = samples;
      st.w = pw;
      st.h = ph;
    }
    e.primed = st.have_bg;
    e.cells = size_t(motion::cells(u32(pw), u32(prm.cell))) * motion::cells(u32(ph), u32(prm.cell));
  }
  void run(std::vector<Eval*>& todo) {
    size_t total_cells = 0;
    for (Eval* e : todo) {
      e->at = total_cells;
      total_cells += e->cells;
    }
    if (!w.dev_.gpu()) {
      for (Eval* e : todo) {
        MotionState& st = e->c->motion;
        e->counts.resize(e->cells);
        motion::update_cpu(e->ring->slot_ptr(e->slot), st.w, st.h, size_t(st.w) * 3, e->primed ? st.bg[st.cur] : nullptr,
                           st.bg[st.cur ^ 1], motion::pitch_for(u32(st.w)), prm.cell, prm.threshold, prm.learn_shift,
                           e->counts.data());
      }
      return;
    }
    w.dev_.bind();
    gpu::MotionPool::Lease set = w.motion_pool_.acquire();
    set->reserve(int(todo.size()), total_cells);
    for (size_t k = 0; k < todo.size(); ++k) {
      Eval& e = *todo[k];
      MotionState& st = e.c->motion;
      set->h_descs.p[k] = gpu::make_motion_desc(
          e.ring->slot_ptr(e.slot), e.ring->slot_bytes(), st.w, st.h, e.primed ? st.bg[st.cur] : nullptr,
          st.bg[st.cur ^ 1], motion::pitch_for(u32(st.w)), st.samples, set->d_counts.p + e.at, e.cells, prm.cell,
          prm.threshold, prm.learn_shift);
    }
    set->run(int(todo.size()), total_cells, w.serve_stream_);
    VEP_HIP(hipEventSynchronize(set->ev));
    const u32* r = set->h_counts.p;
    for (Eval* e : todo) e->counts.assign(r + e->at, r + e->at + e->cells);
  }
  void commit(Eval& e) {  // the slot proved unchanged: only now do the planes swap
    MotionState& st = e.c->motion;
    st.cur ^= 1;
    st.have_bg = true;
    st.seq = e.meta.seq;
    MotionResult& r = st.result;
    r.seq = e.meta.seq;
    r.width = st.w;
    r.height = st.h;
    r.cell = prm.cell;
    r.cols = int(motion::cells(u32(st.w), u32(prm.cell)));
    r.rows = int(motion::cells(u32(st.h), u32(prm.cell)));
    r.threshold = prm.threshold;
    r.primed = e.primed;
    r.counts = std::move(e.counts);
    r.summary = motion::summarize(r.counts.data(), st.w, st.h, prm.cell, prm.cell_percent, prm.min_cells);
    e.c->motion_evaluations.fetch_add(1);
    if (r.summary.motion) e.c->motion_frames.fetch_add(1);
    e.result = r;
  }
};

bool Worker::read_motion(int cam, i64 after, MotionResult& out) {
  MotionOp op{*this};
  return read_camera(*this, op, cam, after, &out);
}

void Worker::read_motion_many(const std::vector<int>& cams, std::vector<MotionResult>& out, std::vector<char>& ok) {
  MotionOp op{*this};
  read_cameras(*this, op, cams, 0, out, ok);
}

// ------------------------------------------------------------------------- tamper detection

void Worker::set_tamper_params(const tamper::Params& p) {
  tamper::check_params(p);
  {
    std::lock_guard<std::mutex> g(tamper_mu_);
    tamper_params_ = p;
    ++tamper_gen_;  // an answer of an older generation counts as none
  }
  std::vector<std::shared_ptr<Camera>> cams;
  {
    std::lock_guard<std::mutex> g(cams_mu_);
    cams = cams_;
  }
  for (auto& c : cams) {
    if (!c) continue;
    TamperState& st = c->tamper;
    std::lock_guard<std::mutex> g(st.mu);
    st.seq = 0;
    st.result = TamperResult{};
    if (st.have_ref && st.ref.cell != p.cell) {
      st.have_ref = false;
      st.ref = tamper::Reference{};
    }
  }
}

tamper::Params Worker::tamper_params() {
  std::lock_guard<std::mutex> g(tamper_mu_);
  return tamper_params_;
}

void Worker::tamper_reset(int cam) {
  std::shared_ptr<Camera> c = camera(cam);
  VEP_CHECK(c, "no such camera");
  TamperState& st = c->tamper;
  std::lock_guard<std::mutex> g(st.mu);
  st.seq = 0;
  st.result = TamperResult{};
  st.have_ref = false;
  st.ref = tamper::Reference{};
}

struct Worker::TamperOp {
  struct Eval : CamEval<TamperResult> {
    int w = 0, h = 0;
    size_t cells = 0;                 // of its grid
    size_t hist_at = 0, grid_at = 0;  // its histogram and its two planes in the request's results
    std::vector<u32> hist, sum_y, energy;
  };
  Worker& w;
  bool set_reference = false;  // the answer, stored or fresh, becomes the camera's reference
  tamper::Params prm;
  u64 gen = 0;
  static TamperState& state(Camera& c) { return c.tamper; }
  static bool live(Camera&) { return true; }
  void snapshot() {
    std::lock_guard<std::mutex> g(w.tamper_mu_);
    prm = w.tamper_params_;
    gen = w.tamper_gen_;
  }
  // The stored answer as the camera's reference, and summarised again against it.
  void make_reference(TamperState& st) {
    const TamperResult& r = st.result;
    st.ref.w = r.width;
    st.ref.h = r.height;
    st.ref.cell = r.cell;
    st.ref.sum_y = r.sum_y;
    st.ref.energy_total = r.summary.energy_total;
    st.have_ref = true;
    st.result.summary = tamper::summarize(r.hist.data(), r.sum_y.data(), r.energy.data(), r.width, r.height, prm, &st.ref);
  }
  bool stored(Eval& e) {
    TamperState& st = e.c->tamper;
    if (st.gen != gen || st.ring.lock() != e.ring) {  // other parameters or a new ring: no stored answer
      st.seq = 0;
      st.result = TamperResult{};
      if (st.have_ref && st.ref.cell != prm.cell) {
        st.have_ref = false;
        st.ref = tamper::Reference{};
      }
      st.gen = gen;
      st.ring = e.ring;
    }
    if (st.seq != e.meta.seq || st.seq == 0) return false;
    if (set_reference) make_reference(st);
    e.result = st.result;  // evaluated already: one evaluation per frame
    return true;
  }
  void plan(Eval& e) {
    e.w = e.ring->width();
    e.h = e.ring->height();
    e.cells = size_t(tamper::cells(u32(e.w), u32(prm.cell))) * tamper::cells(u32(e.h), u32(prm.cell));
  }
  void run(std::vector<Eval*>& todo) {
    const size_t hist_words = todo.size() * size_t(tamper::kBins);
    size_t res_words = hist_words;  // the planes follow the histograms
    for (size_t k = 0; k < todo.size(); ++k) {
      todo[k]->hist_at = k * size_t(tamper::kBins);
      todo[k]->grid_at = res_words;
      res_words += 2 * todo[k]->cells;
    }
    if (!w.dev_.gpu()) {
      for (Eval* e : todo) {
        e->hist.resize(size_t(tamper::kBins));
        e->sum_y.resize(e->cells);
        e->energy.resize(e->cells);
        tamper::stats_cpu(e->ring->slot_ptr(e->slot), e->w, e->h, size_t(e->w) * 3, prm.cell, e->hist.data(),
                          e->sum_y.data(), e->energy.data());
      }
      return;
    }
    w.dev_.bind();
    gpu::TamperPool::Lease set = w.tamper_pool_.acquire();
    set->reserve(int(todo.size()), res_words);
    for (size_t k = 0; k < todo.size(); ++k) {
      Eval& e = *todo[k];
      u32* res = set->d_res.p;
      set->h_descs.p[k] = gpu::make_tamper_desc(e.ring->slot_ptr(e.slot), e.ring->slot_bytes(), e.w, e.h, res + e.hist_at,
                                                res + e.grid_at, res + e.grid_at + e.cells, e.cells, prm.cell);
    }
    set->run(int(todo.size()), hist_words, res_words, w.serve_stream_);
    VEP_HIP(hipEventSynchronize(set->ev));
    const u32* r = set->h_res.p;
    for (Eval* e : todo) {
      e->hist.assign(r + e->hist_at, r + e->hist_at + tamper::kBins);
      e->sum_y.assign(r + e->grid_at, r + e->grid_at + e->cells);
      e->energy.assign(r + e->grid_at + e->cells, r + e->grid_at + 2 * e->cells);
    }
  }
  void commit(Eval& e) {
    TamperState& st = e.c->tamper;
    st.seq = e.meta.seq;
    TamperResult& r = st.result;
    r.seq = e.meta.seq;
    r.width = e.w;
    r.height = e.h;
    r.cell = prm.cell;
    r.cols = int(tamper::cells(u32(e.w), u32(prm.cell)));
    r.rows = int(tamper::cells(u32(e.h), u32(prm.cell)));
    r.hist = std::move(e.hist);
    r.sum_y = std::move(e.sum_y);
    r.energy = std::move(e.energy);
    r.summary = tamper::summarize(r.hist.data(), r.sum_y.data(), r.energy.data(), e.w, e.h, prm,
                                  st.have_ref ? &st.ref : nullptr);
    e.c->tamper_evaluations.fetch_add(1);
    if (r.summary.tampered) e.c->tamper_frames.fetch_add(1);
    if (set_reference) make_reference(st);
    e.result = r;
  }
};

bool Worker::read_tamper(int cam, i64 after, TamperResult& out) {
  TamperOp op{*this};
  return read_camera(*this, op, cam, after, &out);
}

void Worker::read_tamper_many(const std::vector<int>& cams, std::vector<TamperResult>& out, std::vector<char>& ok) {
  TamperOp op{*this};
  read_cameras(*this, op, cams, 0, out, ok);
}

bool Worker::tamper_set_reference(int cam) {
  VEP_CHECK(camera(cam), "no such camera");
  TamperOp op{*this, true};
  return read_camera<TamperOp, TamperResult>(*this, op, cam, 0, nullptr);
}

// ---------------------------------------------------------------------------- motion vectors

void Worker::set_flow_params(const flow::Params& p) {
  flow::check_params(p);
  {
    std::lock_guard<std::mutex> g(flow_mu_);
    flow_params_ = p;
    ++flow_gen_;  // an answer of an older generation counts as none
  }
  std::vector<std::shared_ptr<Camera>> cams;
  {
    std::lock_guard<std::mutex> g(cams_mu_);
    cams = cams_;
  }
  for (auto& c : cams) {
    if (!c) continue;
    std::lock_guard<std::mutex> g(c->flow.mu);
    c->flow.seq = 0;
    c->flow.result = FlowResult{};
  }
}

flow::Params Worker::flow_params() {
  std::lock_guard<std::mutex> g(flow_mu_);
  return flow_params_;
}

struct Worker::FlowOp {
  struct Eval : CamEval<FlowResult, FramesEntry> {
    int w = 0, h = 0;
    bool primed = false;  // the ring held the frame `gap` before the newest, of the same size
    i64 prev_seq = 0;
    size_t blocks = 0;    // of its grid (0 unless primed)
    size_t at = 0;        // its records in the request's
    std::vector<flow::Record> records;
  };
  Worker& w;
  std::vector<Eval>* evs = nullptr;
  flow::Params prm;
  u64 gen = 0;
  static FlowState& state(Camera& c) { return c.flow; }
  static bool live(Camera& c) { return !c.flow.removed; }
  void snapshot() {
    std::lock_guard<std::mutex> g(w.flow_mu_);
    prm = w.flow_params_;
    gen = w.flow_gen_;
    for (Eval& e : *evs) e.frames = prm.gap + 1;
  }
  bool stored(Eval& e) {
    FlowState& st = e.c->flow;
    if (st.gen != gen || st.ring.lock() != e.ring) {  // other parameters or a new ring: no stored answer
      st.seq = 0;
      st.result = FlowResult{};
      st.gen = gen;
      st.ring = e.ring;
    }
    if (st.seq != e.meta.seq || st.seq == 0) return false;
    e.result = st.result;  // evaluated already: one evaluation per frame pair
    return true;
  }
  void plan(Eval& e) {
    VEP_CHECK(e.ring->history() > prm.gap,
              "flow: the camera's ring keeps too little history: buffer.in_memory must be larger than flow.gap");
    e.w = e.ring->width();
    e.h = e.ring->height();
    const size_t gap = size_t(prm.gap);
    e.primed = e.have.size() > gap && e.have[gap].first.width == e.meta.width && e.have[gap].first.height == e.meta.height;
    e.prev_seq = e.primed ? e.have[gap].first.seq : 0;
    // only the slots that are used have to stay valid: the newest, and the earlier one when primed
    if (e.primed) e.have[1] = e.have[gap];
    e.have.resize(e.primed ? 2 : 1);
    const u32 d = u32(prm.decimate);
    e.blocks = e.primed ? size_t(flow::blocks(flow::plane_side(u32(e.w), d))) * flow::blocks(flow::plane_side(u32(e.h), d)) : 0;
  }
  void run(std::vector<Eval*>& todo) {
    size_t records = 0, planes = 0;
    int n = 0;
    for (Eval* e : todo) {
      e->at = records;
      records += e->blocks;
      if (!e->primed) continue;
      planes += gpu::FlowSet::plane_bytes(e->w, e->h, prm.decimate);
      ++n;
    }
    if (!n) return;
    if (!w.dev_.gpu()) {
      std::vector<u8> plane[2];
      for (Eval* e : todo) {
        if (!e->primed) continue;
        const size_t half = gpu::FlowSet::plane_bytes(e->w, e->h, prm.decimate) / 2;
        e->records.assign(std::max<size_t>(e->blocks, 1), flow::Record{});
        flow::Job j;
        for (int k = 0; k < 2; ++k) {
          plane[k].resize(half + 16);
          j.src[k] = e->ring->slot_ptr(e->have[size_t(k)].second);
          j.src_bytes[k] = e->ring->slot_bytes();
          j.src_pitch[k] = u32(e->w) * 3;
          j.plane[k] = plane[k].data() + ((16 - (reinterpret_cast<uintptr_t>(plane[k].data()) & 15u)) & 15u);
          j.plane_bytes[k] = half;
        }
        j.records = e->records.data();
        j.record_count = e->records.size();
        j.w = e->w;
        j.h = e->h;
        j.decimate = prm.decimate;
        j.range = prm.range;
        flow::flow_cpu(j);
        e->records.resize(e->blocks);
      }
      return;
    }
    w.dev_.bind();
    gpu::FlowPool::Lease set = w.flow_pool_.acquire();
    set->reserve(n, planes, records);
    size_t plane_at = 0, record_at = 0;
    int k = 0;
    for (Eval* e : todo) {
      if (!e->primed) continue;
      set->put(k++, e->ring->slot_ptr(e->have[0].second), e->ring->slot_ptr(e->have[1].second), e->ring->slot_bytes(),
               u32(e->w) * 3, u32(e->w) * 3, e->w, e->h, prm.decimate, prm.range, plane_at, record_at);
    }
    set->run(n, prm.decimate, prm.range, records, w.serve_stream_);
    VEP_HIP(hipEventSynchronize(set->ev));
    const flow::Record* r = set->h_records.p;
    for (Eval* e : todo) e->records.assign(r + e->at, r + e->at + e->blocks);
  }
  void commit(Eval& e) {
    FlowState& st = e.c->flow;
    st.seq = e.meta.seq;
    FlowResult& r = st.result;
    r = FlowResult{};
    r.seq = e.meta.seq;
    r.prev_seq = e.prev_seq;
    r.width = e.w;
    r.height = e.h;
    r.decimate = prm.decimate;
    r.range = prm.range;
    r.gap = prm.gap;
    r.primed = e.primed;
    if (e.primed) {
      r.cols = int(flow::blocks(flow::plane_side(u32(e.w), u32(prm.decimate))));
      r.rows = int(flow::blocks(flow::plane_side(u32(e.h), u32(prm.decimate))));
      r.records = std::move(e.records);
      e.c->flow_evaluations.fetch_add(1);
    }
    r.summary = flow::summarize(r.records.data(), r.cols, r.rows, prm.decimate, prm.min_gain, prm.min_blocks, prm.global_percent);
    if (r.summary.motion) e.c->flow_frames.fetch_add(1);
    e.result = r;
  }
};

bool Worker::read_flow(int cam, i64 after, FlowResult& out) {
  std::vector<FlowResult> res;
  std::vector<char> ok;
  FlowOp op{*this};
  read_each_once<FlowOp::Eval>({cam}, after, res, ok, [&](std::vector<FlowOp::Eval>& evs) {
    op.evs = &evs;
    eval_cameras(*this, evs, op);
  });
  if (ok[0]) out = std::move(res[0]);
  return ok[0] != 0;
}

void Worker::read_flow_many(const std::vector<int>& cams, std::vector<FlowResult>& out, std::vector<char>& ok) {
  FlowOp op{*this};
  read_each_once<FlowOp::Eval>(cams, 0, out, ok, [&](std::vector<FlowOp::Eval>& evs) {
    op.evs = &evs;
    eval_cameras(*this, evs, op);
  });
}

// ---------------------------------------------------------------------- moving-object boxes

void Worker::set_objects_params(const objects::Params& p) {
  objects::check_params(p);
  {
    std::lock_guard<std::mutex> g(objects_mu_);
    objects_params_ = p;
    ++objects_gen_;  // an answer of an older generation counts as none
  }
  std::vector<std::shared_ptr<Camera>> cams;
  {
    std::lock_guard<std::mutex> g(cams_mu_);
    cams = cams_;
  }
  for (auto& c : cams) {
    if (!c) continue;
    std::lock_guard<std::mutex> g(c->objects.mu);
    c->objects.seq = 0;
    c->objects.result = ObjectsResult{};
  }
}

objects::Params Worker::objects_params() {
  std::lock_guard<std::mutex> g(objects_mu_);
  return objects_params_;
}

struct Worker::ObjectsOp {
  struct Eval : CamEval<ObjectsResult, FramesEntry> {
    int w = 0, h = 0;
    bool primed = false;  // the ring held the frame `gap` before the newest, of the same size
    i64 prev_seq = 0;
    std::vector<objects::Record> records;
  };
  Worker& w;
  std::vector<Eval>* evs = nullptr;
  objects::Params prm;
  u64 gen = 0;
  static ObjectsState& state(Camera& c) { return c.objects; }
  static bool live(Camera& c) { return !c.objects.removed; }
  void snapshot() {
    std::lock_guard<std::mutex> g(w.objects_mu_);
    prm = w.objects_params_;
    gen = w.objects_gen_;
    for (Eval& e : *evs) e.frames = prm.gap + 1;
  }
  bool stored(Eval& e) {
    ObjectsState& st = e.c->objects;
    if (st.gen != gen || st.ring.lock() != e.ring) {  // other parameters or a new ring: no stored answer
      st.seq = 0;
      st.result = ObjectsResult{};
      st.gen = gen;
      st.ring = e.ring;
    }
    if (st.seq != e.meta.seq || st.seq == 0) return false;
    e.result = st.result;  // evaluated already: one evaluation per frame pair
    return true;
  }
  void plan(Eval& e) {
    VEP_CHECK(e.ring->history() > prm.gap,
              "objects: the camera's ring keeps too little history: buffer.in_memory must be larger than objects.gap");
    e.w = e.ring->width();
    e.h = e.ring->height();
    const size_t gap = size_t(prm.gap);
    e.primed = e.have.size() > gap && e.have[gap].first.width == e.meta.width && e.have[gap].first.height == e.meta.height;
    e.prev_seq = e.primed ? e.have[gap].first.seq : 0;
    // only the slots that are used have to stay valid: the newest, and the earlier one when primed
    if (e.primed) e.have[1] = e.have[gap];
    e.have.resize(e.primed ? 2 : 1);
    e.records.clear();
  }
  void run(std::vector<Eval*>& todo) {
    size_t records = 0, scratch = 0;
    int n = 0;
    for (Eval* e : todo) {
      if (!e->primed) continue;
      scratch += gpu::ObjectsSet::scratch_bytes(e->w, e->h, prm.decimate);
      records += gpu::ObjectsSet::capacity(e->w, e->h, prm.decimate, prm.min_area);
      ++n;
    }
    if (!n) return;
    if (!w.dev_.gpu()) {
      std::vector<u8> planes;
      std::vector<u64> mask;
      std::vector<u32> labels, area;
      for (Eval* e : todo) {
        if (!e->primed) continue;
        const u32 pw = flow::plane_side(u32(e->w), u32(prm.decimate)), ph = flow::plane_side(u32(e->h), u32(prm.decimate));
        const size_t half = size_t(flow::plane_pitch(pw)) * ph;  // (a multiple of 16)
        planes.resize(2 * half + 16);
        mask.resize(size_t(objects::mask_words(pw)) * ph + 1);
        labels.resize(size_t(pw) * ph + 1);
        area.resize(size_t(pw) * ph + 1);
        u8* base = planes.data() + ((16 - (reinterpret_cast<uintptr_t>(planes.data()) & 15u)) & 15u);
        e->records.assign(std::max<size_t>(gpu::ObjectsSet::capacity(e->w, e->h, prm.decimate, prm.min_area), 1), objects::Record{});
        u32 count = 0;
        objects::Job j;
        for (int k = 0; k < 2; ++k) {
          j.src[k] = e->ring->slot_ptr(e->have[size_t(k)].second);
          j.src_bytes[k] = e->ring->slot_bytes();
          j.src_pitch[k] = u32(e->w) * 3;
          j.plane[k] = base + size_t(k) * half;
          j.plane_bytes[k] = half;
        }
        j.mask = mask.data();
        j.mask_count = mask.size();
        j.labels = labels.data();
        j.area = area.data();
        j.sample_count = size_t(pw) * ph;
        j.records = e->records.data();
        j.record_count = e->records.size();
        j.count = &count;
        j.w = e->w;
        j.h = e->h;
        j.decimate = prm.decimate;
        j.threshold = prm.threshold;
        j.open = prm.open;
        j.grow = prm.grow;
        j.min_area = prm.min_area;
        objects::objects_cpu(j);
        e->records.resize(count);
      }
      return;
    }
    w.dev_.bind();
    gpu::ObjectsPool::Lease set = w.objects_pool_.acquire();
    set->reserve(n, scratch, records);
    size_t scratch_at = 0, record_at = 0;
    int k = 0;
    for (Eval* e : todo) {
      if (!e->primed) continue;
      set->put(k++, e->ring->slot_ptr(e->have[0].second), e->ring->slot_ptr(e->have[1].second), e->ring->slot_bytes(),
               u32(e->w) * 3, u32(e->w) * 3, e->w, e->h, prm, scratch_at, record_at);
    }
    set->run(n, prm.decimate, w.serve_stream_);
    VEP_HIP(hipEventSynchronize(set->ev));
    std::vector<size_t> at;
    set->fetch(n, w.serve_stream_, at);
    k = 0;
    for (Eval* e : todo) {
      if (!e->primed) continue;
      e->records.assign(set->h_records.p + at[size_t(k)], set->h_records.p + at[size_t(k) + 1]);
      ++k;
    }
  }
  void commit(Eval& e) {
    ObjectsState& st = e.c->objects;
    st.seq = e.meta.seq;
    ObjectsResult& r = st.result;
    r = ObjectsResult{};
    r.seq = e.meta.seq;
    r.prev_seq = e.prev_seq;
    r.width = e.w;
    r.height = e.h;
    r.decimate = prm.decimate;
    r.gap = prm.gap;
    r.primed = e.primed;
    if (e.primed) {
      r.records = std::move(e.records);
      e.c->objects_evaluations.fetch_add(1);
    }
    r.summary = objects::summarize(r.records.data(), r.records.size(), prm.decimate, prm.max_objects, e.w, e.h);
    if (r.summary.motion) e.c->objects_frames.fetch_add(1);
    e.result = r;
  }
};

bool Worker::read_objects(int cam, i64 after, ObjectsResult& out) {
  std::vector<ObjectsResult> res;
  std::vector<char> ok;
  ObjectsOp op{*this};
  read_each_once<ObjectsOp::Eval>({cam}, after, res, ok, [&](std::vector<ObjectsOp::Eval>& evs) {
    op.evs = &evs;
    eval_cameras(*this, evs, op);
  });
  if (ok[0]) out = std::move(res[0]);
  return ok[0] != 0;
}

void Worker::read_objects_many(const std::vector<int>& cams, std::vector<ObjectsResult>& out, std::vector<char>& ok) {
  ObjectsOp op{*this};
  read_each_once<ObjectsOp::Eval>(cams, 0, out, ok, [&](std::vector<ObjectsOp::Eval>& evs) {
    op.evs = &evs;
    eval_cameras(*this, evs, op);
  });
}

// ------------------------------------------------------------------------------------- crops

static u32 pad_word(const crop::Pad& p) { return u32(p.b) | u32(p.g) << 8 | u32(p.r) << 16; }

// The crop reads as an op of read_consistent_rounds: nothing is stored, every request is produced
// from its slot, all requests of a round in one launch.
struct Worker::CropOp {
  struct Eval : ReadEntry {
    CropRequest* req = nullptr;
  };
  Worker& w;
  int ow, oh, fit;
  crop::Pad pad;
  bool stored(Eval&) { return false; }
  void plan(Eval&) {}
  void run(std::vector<Eval*>& todo) {
    const size_t one = size_t(ow) * size_t(oh) * 3;
    if (!w.dev_.gpu()) {
      for (Eval* e : todo) {
        CropRequest& r = *e->req;
        r.data.resize(r.boxes.size() * one);
        crop::apply_cpu(e->ring->slot_ptr(e->slot), size_t(e->ring->width()) * 3, e->ring->width(), e->ring->height(),
                        r.boxes.data(), int(r.boxes.size()), r.data.data(), ow, oh, fit, pad);
      }
      return;
    }
    size_t nd = 0;
    for (Eval* e : todo) nd += e->req->boxes.size();
    VEP_CHECK(nd <= 65535, "crop: at most 65535 boxes per request");
    for (Eval* e : todo) e->req->data.clear();
    if (!nd) return;
    w.dev_.bind();
    gpu::CropPool::Lease set = w.crop_pool_.acquire();
    set->reserve(int(nd), nd * one, nd * one);
    size_t k = 0;
    for (Eval* e : todo) {
      const FrameRing& ring = *e->ring;
      for (const crop::Box& b : e->req->boxes) {
        set->h_descs.p[k] = gpu::make_crop_desc(ring.slot_ptr(e->slot), ring.slot_bytes(), ring.width(), ring.height(),
                                                crop::to_pixels(ring.width(), ring.height(), b), set->out.p + k * one,
                                                one, ow, oh, fit, pad_word(pad));
        ++k;
      }
    }
    set->run(int(nd), nd * one, w.serve_stream_);
    VEP_HIP(hipEventSynchronize(set->ev));
    k = 0;
    for (Eval* e : todo) {
      const size_t n = e->req->boxes.size();
      e->req->data.assign(set->host.p + k * one, set->host.p + (k + n) * one);
      k += n;
    }
  }
  void commit(Eval& e) {  // the slot proved unchanged
    e.req->meta = e.meta;
    e.req->ok = true;
  }
};

void Worker::read_crops_many(std::vector<CropRequest>& reqs, int ow, int oh, int fit, const crop::Pad& pad) {
  crop::check_output(ow, oh, fit, pad);
  for (CropRequest& r : reqs) {
    crop::check_list(r.boxes.data(), int(r.boxes.size()));
    VEP_CHECK(r.after >= 0 && r.seq >= 0, "crop: after and seq must be >= 0");
    r.ok = false;
    r.data.clear();
  }
  std::vector<CropOp::Eval> evs(reqs.size());
  for (size_t k = 0; k < reqs.size(); ++k) {
    CropOp::Eval& e = evs[k];
    e.req = &reqs[k];
    e.after = reqs[k].after;
    e.seq = reqs[k].seq;
    if (std::shared_ptr<Camera> c = camera(reqs[k].cam)) e.ring = c->ring();
    e.pending = e.ring != nullptr;
  }
  CropOp op{*this, ow, oh, fit, pad};
  read_consistent_rounds(evs, op);
  for (CropRequest& r : reqs)
    if (!r.ok) r.data.clear();  // (produced from a slot that was reused: never returned)
}

bool Worker::read_crops(int cam, i64 after, i64 seq, const std::vector<crop::Box>& boxes, int ow, int oh, int fit,
                        const crop::Pad& pad, FrameMeta* meta, std::vector<u8>& dst) {
  std::vector<CropRequest> reqs(1);
  reqs[0].cam = cam;
  reqs[0].after = after;
  reqs[0].seq = seq;
  reqs[0].boxes = boxes;
  read_crops_many(reqs, ow, oh, fit, pad);
  if (!reqs[0].ok) return false;
  *meta = reqs[0].meta;
  dst.swap(reqs[0].data);
  return true;
}

bool Worker::read_crop_jpeg(int cam, i64 after, i64 seq, const crop::Box& box, int ow, int oh, int fit,
                            const crop::Pad& pad, int quality, FrameMeta* meta, std::string& out) {
  VEP_CHECK(quality >= 1 && quality <= 100, "jpeg: quality must be 1..100");
  crop::check_box(box);
  crop::check_output(ow, oh, fit, pad);
  VEP_CHECK(after >= 0 && seq >= 0, "crop: after and seq must be >= 0");
  std::shared_ptr<Camera> c = camera(cam);
  if (!c) return false;
  std::shared_ptr<FrameRing> ring = c->ring();
  if (!ring) return false;
  const int w = ring->width(), h = ring->height();
  const size_t one = size_t(ow) * size_t(oh) * 3;
  return read_consistent(*ring, after, seq, meta, [&](int slot, const FrameMeta&) {
    if (!dev_.gpu()) {
      std::vector<u8> host(one);
      crop::apply_cpu(ring->slot_ptr(slot), size_t(w) * 3, w, h, &box, 1, host.data(), ow, oh, fit, pad);
      out = jpeg::encode_cpu(host.data(), ow, oh, quality);
      return;
    }
    dev_.bind();
    gpu::CropPool::Lease set = crop_pool_.acquire();
    set->reserve(1, one, 0);
    set->h_descs.p[0] = gpu::make_crop_desc(ring->slot_ptr(slot), ring->slot_bytes(), w, h, crop::to_pixels(w, h, box),
                                            set->out.p, one, ow, oh, fit, pad_word(pad));
    set->run(1, 0, serve_stream_);
    // (the same stream, so the encode is ordered after the crop; it waits for the stream)
    encode_device(set->out.p, ow, oh, quality, out);
  });
}

// ------------------------------------------------------------------------------------- views

static void check_view_request(const std::vector<i32>& mesh, int src_w, int src_h, int ow, int oh, const crop::Pad& pad,
                               i64 after, i64 seq) {
  dewarp::check_output(ow, oh, pad);
  dewarp::check_source(src_w, src_h);
  VEP_CHECK(mesh.size() == size_t(dewarp::mesh_w(ow)) * size_t(dewarp::mesh_h(oh)) * 2,
            "view: the mesh must hold (ceil(width / 8) + 1) * (ceil(height / 8) + 1) pairs");
  VEP_CHECK(after >= 0 && seq >= 0, "view: after and seq must be >= 0");
}

// The view reads as an op of read_consistent_rounds: nothing is stored, every request is produced
// from its slot, all requests of a round in one launch. A frame of another size than the mesh was
// built for produces nothing and commits kViewSize.
struct Worker::ViewOp {
  struct Eval : ReadEntry {
    ViewRequest* req = nullptr;
    bool fits = false;  // the frame has the size the mesh was built for
  };
  Worker& w;
  crop::Pad pad;
  bool stored(Eval&) { return false; }
  void plan(Eval& e) { e.fits = e.ring->width() == e.req->src_w && e.ring->height() == e.req->src_h; }
  void run(std::vector<Eval*>& todo) {
    size_t nd = 0, words = 0, bytes = 0;
    for (Eval* e : todo) {
      e->req->data.clear();
      if (!e->fits) continue;
      ++nd;
      words += e->req->mesh.size();
      bytes += size_t(e->req->ow) * size_t(e->req->oh) * 3;
    }
    if (!nd) return;
    if (!w.dev_.gpu()) {
      for (Eval* e : todo) {
        if (!e->fits) continue;
        ViewRequest& r = *e->req;
        r.data.resize(size_t(r.ow) * size_t(r.oh) * 3);
        dewarp::apply_cpu(e->ring->slot_ptr(e->slot), size_t(r.src_w) * 3, r.src_w, r.src_h, r.mesh.data(), r.ow, r.oh, pad,
                          r.data.data());
      }
      return;
    }
    VEP_CHECK(nd <= 65535, "view: at most 65535 views per request");
    w.dev_.bind();
    gpu::DewarpPool::Lease set = w.dewarp_pool_.acquire();
    set->reserve(int(nd), words, bytes, bytes);
    size_t k = 0, mat = 0, oat = 0;
    for (Eval* e : todo) {
      if (!e->fits) continue;
      const ViewRequest& r = *e->req;
      const FrameRing& ring = *e->ring;
      const size_t one = size_t(r.ow) * size_t(r.oh) * 3;
      std::memcpy(set->h_mesh.p + mat, r.mesh.data(), r.mesh.size() * sizeof(i32));
      set->h_descs.p[k++] = gpu::make_dewarp_desc(ring.slot_ptr(e->slot), ring.slot_bytes(), r.src_w, r.src_h,
                                                  set->d_mesh.p + mat, r.mesh.size() / 2, set->out.p + oat, one, r.ow,
                                                  r.oh, pad_word(pad));
      mat += r.mesh.size();
      oat += one;
    }
    set->run(int(nd), words, bytes, w.serve_stream_);
    VEP_HIP(hipEventSynchronize(set->ev));
    oat = 0;
    for (Eval* e : todo) {
      if (!e->fits) continue;
      const size_t one = size_t(e->req->ow) * size_t(e->req->oh) * 3;
      e->req->data.assign(set->host.p + oat, set->host.p + oat + one);
      oat += one;
    }
  }
  void commit(Eval& e) {  // the slot proved unchanged
    e.req->meta = e.meta;
    e.req->status = e.fits ? kViewOk : kViewSize;
  }
};

void Worker::read_views_many(std::vector<ViewRequest>& reqs, const crop::Pad& pad) {
  for (ViewRequest& r : reqs) {
    check_view_request(r.mesh, r.src_w, r.src_h, r.ow, r.oh, pad, r.after, r.seq);
    r.status = kViewNone;
    r.data.clear();
  }
  std::vector<ViewOp::Eval> evs(reqs.size());
  for (size_t k = 0; k < reqs.size(); ++k) {
    ViewOp::Eval& e = evs[k];
    e.req = &reqs[k];
    e.after = reqs[k].after;
    e.seq = reqs[k].seq;
    if (std::shared_ptr<Camera> c = camera(reqs[k].cam)) e.ring = c->ring();
    e.pending = e.ring != nullptr;
  }
  ViewOp op{*this, pad};
  read_consistent_rounds(evs, op);
  for (ViewRequest& r : reqs)
    if (r.status != kViewOk) r.data.clear();  // (produced from a slot that was reused: never returned)
}

int Worker::read_view(int cam, i64 after, i64 seq, const std::vector<i32>& mesh, int src_w, int src_h, int ow, int oh,
                      const crop::Pad& pad, FrameMeta* meta, std::vector<u8>& dst) {
  std::vector<ViewRequest> reqs(1);
  ViewRequest& r = reqs[0];
  r.cam = cam;
  r.after = after;
  r.seq = seq;
  r.mesh = mesh;
  r.src_w = src_w, r.src_h = src_h, r.ow = ow, r.oh = oh;
  read_views_many(reqs, pad);
  if (r.status != kViewNone) *meta = r.meta;
  if (r.status == kViewOk) dst.swap(r.data);
  return r.status;
}

int Worker::read_view_jpeg(int cam, i64 after, i64 seq, const std::vector<i32>& mesh, int src_w, int src_h, int ow, int oh,
                           const crop::Pad& pad, int quality, FrameMeta* meta, std::string& out) {
  VEP_CHECK(quality >= 1 && quality <= 100, "jpeg: quality must be 1..100");
  check_view_request(mesh, src_w, src_h, ow, oh, pad, after, seq);
  std::shared_ptr<Camera> c = camera(cam);
  if (!c) return kViewNone;
  std::shared_ptr<FrameRing> ring = c->ring();
  if (!ring) return kViewNone;
  if (ring->width() != src_w || ring->height() != src_h) {
    int slot;
    return pick_frame(*ring, after, seq, meta, &slot) ? kViewSize : kViewNone;
  }
  const size_t one = size_t(ow) * size_t(oh) * 3;
  const bool ok = read_consistent(*ring, after, seq, meta, [&](int slot, const FrameMeta&) {
    if (!dev_.gpu()) {
      std::vector<u8> host(one);
      dewarp::apply_cpu(ring->slot_ptr(slot), size_t(src_w) * 3, src_w, src_h, mesh.data(), ow, oh, pad, host.data());
      out = jpeg::encode_cpu(host.data(), ow, oh, quality);
      return;
    }
    dev_.bind();
    gpu::DewarpPool::Lease set = dewarp_pool_.acquire();
    set->reserve(1, mesh.size(), one, 0);
    std::memcpy(set->h_mesh.p, mesh.data(), mesh.size() * sizeof(i32));
    set->h_descs.p[0] = gpu::make_dewarp_desc(ring->slot_ptr(slot), ring->slot_bytes(), src_w, src_h, set->d_mesh.p,
                                              mesh.size() / 2, set->out.p, one, ow, oh, pad_word(pad));
    set->run(1, mesh.size(), 0, serve_stream_);
    // (the same stream, so the encode is ordered after the remap; it waits for the stream)
    encode_device(set->out.p, ow, oh, quality, out);
  });
  return ok ? kViewOk : kViewNone;
}

void Worker::copy_slot(FrameRing& ring, int slot, u8* dst) {
  const size_t n = ring.slot_bytes();
  if (!dev_.gpu()) {
    std::memcpy(dst, ring.slot_ptr(slot), n);
    return;
  }
  dev_.bind();
  ServePool::Lease b = serve_pool_->acquire();  // D2H through a pinned pool buffer, as read_latest
  b->reserve(dev_, n);
  VEP_HIP(hipMemcpyAsync(b->h, ring.slot_ptr(slot), n, hipMemcpyDeviceToHost, serve_stream_));
  VEP_HIP(hipEventRecord(b->ev[0], serve_stream_));
  VEP_HIP(hipEventSynchronize(b->ev[0]));
  std::memcpy(dst, b->h, n);
}

std::vector<Worker::HistoryFrame> Worker::read_history(int cam, i64 after, int max_count) {
  std::vector<HistoryFrame> res;
  std::shared_ptr<Camera> c = camera(cam);
  if (!c) return res;
  std::shared_ptr<FrameRing> r = c->ring();
  if (!r) return res;
  // (a ring without a history keeps only its newest frame readable)
  const int depth = std::max(1, r->history());
  std::vector<std::pair<FrameMeta, int>> want;
  r->range(after, max_count > 0 ? std::min(max_count, depth) : depth, want);
  // newest first: a frame the writer took meanwhile ends the run (it and everything older is
  // dropped, so the result stays contiguous and ends at the newest frame read)
  for (size_t k = want.size(); k-- > 0;) {
    HistoryFrame f;
    f.meta = want[k].first;
    f.bytes = r->slot_bytes();
    f.data.reset(new u8[f.bytes]);
    copy_slot(*r, want[k].second, f.data.get());
    if (!r->still_valid(want[k].second, f.meta.seq)) break;
    res.push_back(std::move(f));
  }
  std::reverse(res.begin(), res.end());
  return res;
}

void Worker::ServeBuf::reserve(Device& d, size_t n) {
  dev = &d;
  if (cap < n) {  // first use, or a larger ring (resolution change)
    d.free_pinned(h);
    h = nullptr;
    cap = 0;
    h = static_cast<u8*>(d.alloc_pinned(n));
    cap = n;
  }
  if (d.gpu())
    for (gpu::SetEvent& e : ev) e.ensure();
}

Worker::ServeBuf::~ServeBuf() {
  if (dev) dev->free_pinned(h);
}

bool Worker::register_host(void* p, size_t n) {
  if (!dev_.gpu() || !p || !n) return false;
  dev_.bind();
  if (hipHostRegister(p, n, hipHostRegisterDefault) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  return true;
}

void Worker::unregister_host(void* p) {
  if (!dev_.gpu() || !p) return;
  dev_.bind();
  (void)hipHostUnregister(p);
}

bool Worker::read_latest(FrameRing& ring, i64 after, FrameMeta* meta, u8* dst, size_t cap, bool dst_pinned) {
  const size_t n = ring.slot_bytes();
  const bool gpu = dev_.gpu();
  return read_consistent(ring, after, meta, [&](int slot, const FrameMeta&) {
    VEP_CHECK(cap >= n, "read_latest destination too small");
    const u8* src = ring.slot_ptr(slot);
    if (!gpu && !mock_serve_) {
      std::memcpy(dst, src, n);
      return;
    }
    if (gpu) dev_.bind();
    ServePool::Lease b = serve_pool_->acquire();
    if (gpu && dst_pinned) {  // only the buffer's completion event: the DMA lands in dst
      b->reserve(dev_, 0);
      VEP_HIP(hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToHost, serve_stream_));
      VEP_HIP(hipEventRecord(b->ev[0], serve_stream_));
      VEP_HIP(hipEventSynchronize(b->ev[0]));
      return;
    }
    b->reserve(dev_, n);  // (mock: the same pool and chunking, memcpy for the DMA)
    const size_t chunk = (n + kServeChunks - 1) / kServeChunks;
    for (int k = 0; k < kServeChunks; ++k) {
      const size_t off = size_t(k) * chunk;
      if (off >= n) break;
      if (!gpu) {
        std::memcpy(b->h + off, src + off, std::min(chunk, n - off));
        continue;
      }
      VEP_HIP(hipMemcpyAsync(b->h + off, src + off, std::min(chunk, n - off), hipMemcpyDeviceToHost, serve_stream_));
      VEP_HIP(hipEventRecord(b->ev[k], serve_stream_));
    }
    for (int k = 0; k < kServeChunks; ++k) {
      const size_t off = size_t(k) * chunk;
      if (off >= n) break;
      if (gpu) VEP_HIP(hipEventSynchronize(b->ev[k]));
      std::memcpy(dst + off, b->h + off, std::min(chunk, n - off));
    }
  });
}

void Worker::read_latest_many(std::vector<ReadReq>& reqs) {
  if (!dev_.gpu()) {
    for (auto& r : reqs) r.ok = read_latest(*r.ring, r.after, &r.meta, r.dst, r.cap, r.pinned);
    return;
  }
  dev_.bind();
  std::vector<int> slot(reqs.size(), -1);
  bool queued = false;
  for (size_t k = 0; k < reqs.size(); ++k) {
    ReadReq& r = reqs[k];
    r.ok = false;
    if (!r.pinned) {
      r.ok = read_latest(*r.ring, r.after, &r.meta, r.dst, r.cap, false);
      continue;
    }
    if (!r.ring->latest(r.after, &r.meta, &slot[k])) continue;
    VEP_CHECK(r.cap >= r.ring->slot_bytes(), "read_latest_many destination too small");
    VEP_HIP(hipMemcpyAsync(r.dst, r.ring->slot_ptr(slot[k]), r.ring->slot_bytes(), hipMemcpyDeviceToHost,
                           serve_stream_));
    queued = true;
  }
  if (!queued) return;
  {
    ServePool::Lease b = serve_pool_->acquire();  // (its completion event)
    b->reserve(dev_, 0);
    VEP_HIP(hipEventRecord(b->ev[0], serve_stream_));
    VEP_HIP(hipEventSynchronize(b->ev[0]));
  }
  for (size_t k = 0; k < reqs.size(); ++k)  // a slot the writer reused meanwhile is not served
    if (slot[k] >= 0) reqs[k].ok = reqs[k].ring->still_valid(slot[k], reqs[k].meta.seq);
}

// --------------------------------------------------------------------------- proto encoding

static void put_varint(std::string& s, u64 v) {
  while (v >= 0x80) {
    s.push_back(char((v & 0x7f) | 0x80));
    v >>= 7;
  }
  s.push_back(char(v));
}
static void put_tag(std::string& s, int field, int wt) { put_varint(s, u64(field) << 3 | u64(wt)); }
static void put_i64(std::string& s, int field, i64 v) {
  if (v == 0) return;
  put_tag(s, field, 0);
  put_varint(s, u64(v));
}
static void put_bool(std::string& s, int field, bool v) {
  if (!v) return;
  put_tag(s, field, 0);
  s.push_back(1);
}
static void put_str(std::string& s, int field, const std::string& v) {
  if (v.empty()) return;
  put_tag(s, field, 2);
  put_varint(s, v.size());
  s += v;
}

std::pair<std::string, std::string> encode_video_frame(const FrameMeta& m, size_t data_len,
                                                       const std::string& device_id) {
  std::string pre, suf;
  put_i64(pre, 1, m.width);
  put_i64(pre, 2, m.height);
  if (data_len) {
    put_tag(pre, 3, 2);
    put_varint(pre, data_len);
  }
  put_i64(suf, 4, m.timestamp);
  put_bool(suf, 5, m.is_keyframe);
  put_i64(suf, 6, m.pts);
  put_i64(suf, 7, m.dts);
  if (m.frame_type != '?' && m.frame_type != 0) put_str(suf, 8, std::string(1, m.frame_type));
  put_bool(suf, 9, m.is_corrupt);
  if (m.time_base != 0.0) {
    put_tag(suf, 10, 1);
    u64 bits;
    std::memcpy(&bits, &m.time_base, 8);
    for (int i = 0; i < 8; ++i) suf.push_back(char((bits >> (8 * i)) & 0xff));
  }
  if (m.width > 0) {  // ShapeProto{dim: [(H,"0"), (W,"1"), (3,"2")]}
    std::string shape;
    const i64 dims[3] = {m.height, m.width, 3};
    for (int k = 0; k < 3; ++k) {
      std::string dim;
      put_i64(dim, 1, dims[k]);
      put_str(dim, 2, std::string(1, char('0' + k)));
      put_tag(shape, 2, 2);
      put_varint(shape, dim.size());
      shape += dim;
    }
    put_tag(suf, 11, 2);
    put_varint(suf, shape.size());
    suf += shape;
  }
  put_str(suf, 12, device_id);
  put_i64(suf, 13, m.packet);
  put_i64(suf, 14, m.keyframe);
  return {pre, suf};
}

}  // namespace vep
