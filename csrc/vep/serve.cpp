// The serving reads: the Worker methods that answer a client from a camera's ring (frames, scaled
// frames, JPEGs, the wall, history, motion, tamper and crops), the serve-buffer pool they copy
// through, and the VideoFrame wire encoding. Every read follows the consistent-read rule of
// ring_read.h.
#include <algorithm>
#include <cstring>

#include "crop.h"
#include "jpeg.h"
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
  gpu::ScaleDesc& d = set.h_descs.p[0];
  d = gpu::ScaleDesc{};
  d.src = ring.slot_ptr(slot);
  d.sw = ring.width();
  d.sh = ring.height();
  d.src_pitch = u32(ring.width()) * 3;
  d.dst = set.canvas.p;
  d.dst_pitch = u32(ow) * 3;
  d.ow = ow;
  d.oh = oh;
  gpu::check_scale(d, ow, oh);
  set.run(1, serve_stream_);
}

// The newest frame with seq > after, fitted into width x height: consume(set, host, f) gets the
// f.w x f.h picture, on a GPU in set->canvas (scaled on the serving stream, not waited for; the
// set has `download` times its bytes of pinned room), on the CPU backend in `host` (set null).
template <class Consume>
bool Worker::read_scaled(int cam, i64 after, int width, int height, bool download, FrameMeta* meta, Consume&& consume) {
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
      consume(set.get(), host, f);
    } else {
      host.resize(n);
      scale::area_cpu(ring->slot_ptr(slot), ring->width(), ring->height(), size_t(ring->width()) * 3, host.data(),
                      size_t(f.w) * 3, f.w, f.h);
      consume(nullptr, host, f);
    }
  });
  if (ok) {
    meta->width = f.w;
    meta->height = f.h;
  }
  return ok;
}

bool Worker::read_latest_scaled(int cam, i64 after, int width, int height, FrameMeta* meta, std::vector<u8>& dst) {
  return read_scaled(cam, after, width, height, true, meta, [&](gpu::ScaleSet* set, std::vector<u8>& host, scale::Size f) {
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

bool Worker::read_latest_jpeg(int cam, i64 after, int quality, FrameMeta* meta, std::string& out, int width,
                              int height) {
  VEP_CHECK(quality >= 1 && quality <= 100, "jpeg: quality must be 1..100");
  if (width || height)
    return read_scaled(cam, after, width, height, false, meta,
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
                               const std::string& name, FrameMeta* meta, std::string& out, int width, int height) {
  VEP_CHECK(quality >= 1 && quality <= 100, "jpeg: quality must be 1..100");
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
      if (scaled) {
        scale::area_cpu(ring->slot_ptr(slot), w, h, size_t(w) * 3, host.data(), row, f.w, f.h);
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
    // (every request takes its sets in one order: scale, overlay, encoder)
    gpu::ScalePool::Lease set;
    if (scaled) {
      set = scale_pool_.acquire();
      set->reserve(n, 1, 0);
    }
    gpu::OverlayPool::Lease osd = overlay_pool_.acquire();
    osd->reserve(1, e.prims.size(), e.text.size(), scaled ? 0 : n);
    size_t prim_at = 0, text_at = 0;
    if (scaled) {
      scale_slot(*set, *ring, slot, f.w, f.h);
      // (the same stream: drawn after the scale, encoded after the drawing)
      osd->put(0, set->canvas.p, n, u32(row), set->canvas.p, n, u32(row), f.w, f.h, e, prim_at, text_at);
      osd->run(1, prim_at, text_at, serve_stream_);
      encode_device(set->canvas.p, f.w, f.h, quality, out);
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
template <class Result>
struct CamEval : ReadEntry {
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
