// Device-side visualizer: boxes, half-transparent masks with outlines, "NAME score%" labels and keypoints drawn onto a uint8 (H,W,3)
// image (the reference's visualizer.py:21-38 hands the Instances to detectron2's matplotlib Visualizer on the host; the picture here is
// this package's own, defined in integer arithmetic so that a NumPy restatement agrees byte for byte: DESIGN §3 "Visualizer").
//
//   prepare  : vis_prepare_kernel   — one thread per instance in draw order: integer box rect, label glyphs, plate rect, the three colours,
//                                     VIS_REC int32 per instance.  Nothing about an instance is computed on the host.
//   compose  : vis_compose_kernel   — one wave per 64-pixel word of the packed masks (cmk_mask_pack_bits), lane = pixel.  Per 64 instances
//                                     every lane tests ONE instance against the word (its mask word non-zero, or the word's pixel span
//                                     meets the rect around its box and plate) and keeps that instance's record, word and neighbour
//                                     windows in its registers; a ballot leaves the instances that touch the word, and only those are
//                                     walked, in draw order, their values read from the holding lane: no memory latency in the walk.
//                                     The outline needs the bits at p-1, p+1, p-W, p+W: four 64-bit windows cut from at most two words
//                                     each, whatever W % 64 is.  The pixels of a full word are 192 contiguous bytes: 48 lanes move them
//                                     as dwords and the wave redistributes them with two shuffles each way; the last, partial word
//                                     moves bytes.
//   keypoints: vis_kp_clear_kernel  — zeroes the int32 (H,W) winner map;
//              vis_kp_raise_kernel  — one workgroup per primitive (skeleton segment or keypoint disc): atomicMax of its sequence number
//                                     into the winner map over the primitive's own bounding box;
//              vis_kp_colour_kernel — one pass over the winner map colours the pixels some primitive won.  The latest primitive wins a
//                                     pixel whatever the order of the atomics.
//   video    : vis_track_iou_kernel    — box mode: one thread per (old row, new instance), the float64 IoU table;
//              vis_track_assign_kernel — ONE workgroup of 16 waves matches a frame's instances to the track table (DESIGN §3 "Video"):
//                                        a wave per old row finds the first maximum of its row, candidates claim their instance with an
//                                        integer atomicMin in LDS (the smallest old index wins whatever the order), two ballot scans
//                                        number the unmatched instances (new ids) and the surviving missed rows (slots of the next table);
//              vis_track_gather_kernel — mask mode: the packed words and areas of the next table, row by row from the new instances or
//                                        the old table, into the other half of the ping-pong pair.
//              The counters (n_tracks, next_id, dropped) stay on the device; nothing is read back.
//   contours : the exact outlines of the packed masks as loops of lattice vertices (DESIGN §3 "Contours"), two phases around one host read:
//              vis_contour_count_kernel   — a thread per 64 vertices of a lattice row: corner and saddle bits from four shifted row windows,
//                                           their popcounts scanned over 1024 such words in the same pass;
//              vis_contour_offsets_kernel — ONE workgroup scans the block totals of all masks: record numbers, offsets, totals per mask;
//              vis_contour_emit_kernel    — the corner records (x, y, out direction, mask) in lattice row-major order = canonical order;
//              vis_contour_link_kernel    — a wave per record: a horizontal edge ends at record i ^ 1, a vertical one is followed 64 rows
//                                           per ballot to the next corner of its column;
//              vis_contour_jump_kernel    — pointer jumping, one launch per round between ping-pong buffers: the smallest record of every
//                                           loop (its start) and the steps to it;
//              vis_contour_lens_kernel, vis_contour_blocks_kernel, vis_contour_place_kernel — the loop lengths scanned in three launches:
//                                           where every loop goes; vis_contour_write_kernel puts every vertex there.
//              No kernel waits for another workgroup; every loop's trip count is bounded by an argument.
// Every store is an ordinary vector store, the atomics are vector atomics.
#include "cmk_common.hpp"

namespace cmk {

constexpr int VIS_REC = 28;          // int32 per instance record, a multiple of 4: every record is 16-byte aligned
// record layout
constexpr int VR_HIT = 0;            // hx0, hy0, hx1, hy1: the rect that holds box and plate (empty without a box)
constexpr int VR_SRC = 4;            // original index of the instance (its mask words, its keypoints)
constexpr int VR_FLAGS = 5;          // bit 0: box and label are drawn (no NaN coordinate)
constexpr int VR_LEN = 6;            // label length, <= 32
constexpr int VR_COL = 7;            // col: bytes 0..2 are the image's channels 0..2
constexpr int VR_BOX = 8;            // bx0, by0, bx1, by1 (inclusive, unclipped)
constexpr int VR_PLATE = 12;         // px0, py0, pw, ph
constexpr int VR_EDGE = 16;          // edge, text colours, two spare ints
constexpr int VR_TEXT = 17;
constexpr int VR_GLYPH = 20;         // 32 glyph indices as bytes, 8 ints
constexpr int VIS_GLYPHS = 41, VIS_G_SPACE = 0, VIS_G_0 = 1, VIS_G_C = 13, VIS_G_PCT = 37, VIS_G_MINUS = 39;     // glyph 40 is "?"

__device__ inline int vis_floor_clamped(float v, float lim) { return (int)floorf(fminf(fmaxf(v, -lim), lim)); }
__device__ inline int vis_clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ inline int vis_pack3(int a, int b, int c) { return a | (b << 8) | (c << 16); }

__device__ inline void vis_put(uint8_t* g, int& len, int glyph) {
    if (len < 32) g[len++] = (uint8_t)glyph;
}
__device__ inline void vis_put_decimal(uint8_t* g, int& len, unsigned long long v) {
    unsigned long long div = 1;
    while (v / div >= 10) div *= 10;
    for (; div; div /= 10) vis_put(g, len, VIS_G_0 + (int)(v / div % 10));
}

// grid = ceil(n / 64)
__global__ __launch_bounds__(64) void vis_prepare_kernel(const float* __restrict__ boxes, const float* __restrict__ scores, const long long* __restrict__ classes,
                                                        const long long* __restrict__ order, const uint8_t* __restrict__ names,
                                                        const int32_t* __restrict__ name_lens, int num_names, const uint8_t* __restrict__ palette, int n,
                                                        int H, int W, int scale, int by_class, const int32_t* __restrict__ color_ids,
                                                        int32_t* __restrict__ records) {
    const int j = blockIdx.x * 64 + threadIdx.x;
    if (j >= n) return;
    long long src = order[j];
    if (src < 0 || src >= n) src = j;                               // never read outside the inputs, whatever `order` holds
    int32_t* r = records + (long)j * VIS_REC;
    const long long cls = classes[src];

    const long long k = color_ids ? (long long)color_ids[src] : (by_class ? cls : src);    // color_ids: the caller's colour index (track ids)
    const uint8_t* pal = palette + 3 * (int)(((k % 64) + 64) % 64);
    int col[3], edge[3], text[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        col[c] = pal[c];
        edge[c] = (col[c] * 154) >> 8;
        text[c] = col[c] + (((255 - col[c]) * 179) >> 8);
    }
    r[VR_COL] = vis_pack3(col[0], col[1], col[2]);
    r[VR_EDGE] = vis_pack3(edge[0], edge[1], edge[2]);
    r[VR_TEXT] = vis_pack3(text[0], text[1], text[2]);
    r[VR_TEXT + 1] = r[VR_TEXT + 2] = 0;
    r[VR_SRC] = (int)src;

    // label: NAME + " " + P + "%"
#pragma unroll
    for (int i = 0; i < 8; ++i) r[VR_GLYPH + i] = 0;
    uint8_t* g = (uint8_t*)(r + VR_GLYPH);
    int len = 0;
    if (cls >= 0 && cls < num_names) {
        const int nl = min(max(name_lens[cls], 0), 32);
        for (int i = 0; i < nl; ++i) vis_put(g, len, min((int)names[cls * 32 + i], VIS_GLYPHS - 1));
    } else {
        vis_put(g, len, VIS_G_C);
        if (cls < 0) vis_put(g, len, VIS_G_MINUS);
        vis_put_decimal(g, len, cls < 0 ? 0ull - (unsigned long long)cls : (unsigned long long)cls);
    }
    const double sc = (double)scores[src];                          // float32 * 100 is exact in float64: contraction changes nothing
    const double pf = floor(sc * 100.0 + 0.5);
    const int pct = sc != sc ? 0 : (pf < 0.0 ? 0 : (pf > 100.0 ? 100 : (int)pf));
    vis_put(g, len, VIS_G_SPACE);
    vis_put_decimal(g, len, (unsigned long long)pct);
    vis_put(g, len, VIS_G_PCT);
    r[VR_LEN] = len;

    const float x1 = boxes[src * 4], y1 = boxes[src * 4 + 1], x2 = boxes[src * 4 + 2], y2 = boxes[src * 4 + 3];
    const bool nan = x1 != x1 || y1 != y1 || x2 != x2 || y2 != y2;
    const float lim = 1048576.f;
    const int bx0 = nan ? 0 : vis_floor_clamped(x1, lim), by0 = nan ? 0 : vis_floor_clamped(y1, lim);
    const int bx1 = nan ? -1 : vis_floor_clamped(x2, lim), by1 = nan ? -1 : vis_floor_clamped(y2, lim);
    const int pw = (6 * len + 1) * scale, ph = 9 * scale;
    r[VR_FLAGS] = nan ? 0 : 1;
    r[VR_BOX] = bx0, r[VR_BOX + 1] = by0, r[VR_BOX + 2] = bx1, r[VR_BOX + 3] = by1;
    r[VR_PLATE] = vis_clampi(bx0, 0, max(0, W - pw));
    r[VR_PLATE + 1] = vis_clampi(by0, 0, max(0, H - ph));
    r[VR_PLATE + 2] = pw, r[VR_PLATE + 3] = ph;
    r[VR_HIT] = nan ? 0 : min(bx0, r[VR_PLATE]), r[VR_HIT + 1] = nan ? 0 : min(by0, r[VR_PLATE + 1]);
    r[VR_HIT + 2] = nan ? -1 : max(bx1, r[VR_PLATE] + pw - 1), r[VR_HIT + 3] = nan ? -1 : max(by1, r[VR_PLATE + 1] + ph - 1);
}

// 64 mask bits starting at bit position q of a packed mask (wave-uniform); positions outside [0, 64 * nw) read as zero, as the tail does
__device__ inline unsigned long long vis_bits64(const unsigned long long* __restrict__ w, long q, int nw) {
    if (q <= -64 || q >= (long)nw * 64) return 0ull;
    const long wi = q >> 6;                                          // floor: -1 for q in [-63, -1]
    const int sh = (int)(q & 63);
    const unsigned long long lo = wi >= 0 ? w[wi] : 0ull;
    if (!sh) return lo;
    const unsigned long long hi = wi + 1 < nw ? w[wi + 1] : 0ull;
    return (lo >> sh) | (hi << (64 - sh));
}

// does the rect [x0, x1] x [y0, y1] meet the pixel span (columns [sx0, sx1] of rows [sy0, sy1])
__device__ inline bool vis_meets(int x0, int y0, int x1, int y1, int sx0, int sy0, int sx1, int sy1) {
    return x0 <= sx1 && x1 >= sx0 && y0 <= sy1 && y1 >= sy0;
}

// the value lane l (wave-uniform) holds
__device__ inline int vis_lane(int v, int l) { return __builtin_amdgcn_readlane(v, l); }
__device__ inline unsigned long long vis_lane(unsigned long long v, int l) {
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, l), hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), l);
    return ((unsigned long long)hi << 32) | lo;
}

// grid = ceil(nw / 4), 4 independent waves per workgroup; words may be null (no masks); vec: both images are 4-byte aligned
__global__ __launch_bounds__(256) void vis_compose_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, int H, int W, int nw,
                                                         const unsigned long long* __restrict__ words, const int32_t* __restrict__ recs, int n,
                                                         const uint8_t* __restrict__ font, int lw, int s, int A, int vec) {
    const int lane = threadIdx.x & 63;
    const int wi = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
    if (wi >= nw) return;
    const long HW = (long)H * W;
    const long p0 = (long)wi * 64, p = p0 + lane;
    const bool full = vec && p0 + 64 <= HW;                          // wave-uniform
    const int y = (int)(p / W), x = (int)(p - (long)y * W);

    int c0 = 0, c1 = 0, c2 = 0;
    if (full) {
        const uint32_t d = lane < 48 ? reinterpret_cast<const uint32_t*>(in + p0 * 3)[lane] : 0u;
        const int di = (lane * 3) >> 2, sh = ((lane * 3) & 3) * 8;
        const unsigned long long ab = (unsigned long long)__shfl(d, di, 64) | ((unsigned long long)__shfl(d, (di + 1) & 63, 64) << 32);
        const unsigned pix = (unsigned)(ab >> sh);
        c0 = pix & 255, c1 = (pix >> 8) & 255, c2 = (pix >> 16) & 255;
    } else if (p < HW) {
        c0 = in[p * 3], c1 = in[p * 3 + 1], c2 = in[p * 3 + 2];
    }

    // the word's pixel span, wave-uniform
    const long plast = min(p0 + 63, HW - 1);
    const int sy0 = (int)(p0 / W), sy1 = (int)(plast / W);
    const int sx0 = sy0 == sy1 ? (int)(p0 - (long)sy0 * W) : 0, sx1 = sy0 == sy1 ? (int)(plast - (long)sy1 * W) : W - 1;

    for (int j0 = 0; j0 < n; j0 += 64) {
        // lane l holds instance j0 + l: its record as five int4, its word here and the four neighbour windows; does it touch this word
        int4 q0 = {0, 0, -1, -1}, q1 = {0, 0, 0, 0}, qb = q0, qp = q1, qe = q1;
        unsigned long long mine = 0ull, up = 0ull, down = 0ull, left = 0ull, right = 0ull;
        if (j0 + lane < n) {
            const int4* r = reinterpret_cast<const int4*>(recs + (long)(j0 + lane) * VIS_REC);
            q0 = r[0], q1 = r[1], qb = r[2], qp = r[3], qe = r[4];
            if (words) {
                const unsigned long long* w = words + (long)q1.x * nw;
                mine = w[wi];
                if (mine) {
                    up = vis_bits64(w, p0 - W, nw), down = vis_bits64(w, p0 + W, nw);
                    left = vis_bits64(w, p0 - 1, nw), right = vis_bits64(w, p0 + 1, nw);
                }
            }
        }
        unsigned long long todo = __ballot(mine != 0ull || vis_meets(q0.x, q0.y, q0.z, q0.w, sx0, sy0, sx1, sy1));
        while (todo) {                                               // wave-uniform walk in draw order, no memory in it but the glyphs
            const int l = __builtin_ctzll(todo);
            todo &= todo - 1;
            const unsigned long long M = vis_lane(mine, l);
            const int flags = vis_lane(q1.y, l), col = vis_lane(q1.w, l);
            if (flags & 1) {
                const int bx0 = vis_lane(qb.x, l), by0 = vis_lane(qb.y, l), bx1 = vis_lane(qb.z, l), by1 = vis_lane(qb.w, l);
                if (x >= bx0 && x <= bx1 && y >= by0 && y <= by1 && (x - bx0 < lw || bx1 - x < lw || y - by0 < lw || by1 - y < lw))
                    c0 = col & 255, c1 = (col >> 8) & 255, c2 = (col >> 16) & 255;
            }
            if (M) {
                const unsigned long long U = vis_lane(up, l), D = vis_lane(down, l), L = vis_lane(left, l), R = vis_lane(right, l);
                if ((M >> lane) & 1) {
                    c0 = (c0 * (256 - A) + (col & 255) * A + 128) >> 8;
                    c1 = (c1 * (256 - A) + ((col >> 8) & 255) * A + 128) >> 8;
                    c2 = (c2 * (256 - A) + ((col >> 16) & 255) * A + 128) >> 8;
                    const bool inner = ((U >> lane) & 1) && ((D >> lane) & 1) && x > 0 && ((L >> lane) & 1) && x < W - 1 && ((R >> lane) & 1);
                    if (!inner) {
                        const int e = vis_lane(qe.x, l);
                        c0 = e & 255, c1 = (e >> 8) & 255, c2 = (e >> 16) & 255;
                    }
                }
            }
            if (flags & 1) {
                const int lx = x - vis_lane(qp.x, l), ly = y - vis_lane(qp.y, l);
                if (lx >= 0 && lx < vis_lane(qp.z, l) && ly >= 0 && ly < vis_lane(qp.w, l)) {
                    c0 = (c0 * 51 + 128) >> 8, c1 = (c1 * 51 + 128) >> 8, c2 = (c2 * 51 + 128) >> 8;
                    const int cx = lx / s - 1, cy = ly / s - 1;
                    if (cx >= 0 && cy >= 0 && cy < 7) {
                        const int gj = cx / 6, gc = cx - gj * 6;
                        if (gj < vis_lane(q1.z, l) && gj < 32 && gc < 5) {
                            const uint8_t* glyphs = reinterpret_cast<const uint8_t*>(recs + (long)(j0 + l) * VIS_REC + VR_GLYPH);
                            const int g = min((int)glyphs[gj], VIS_GLYPHS - 1);
                            if ((font[g * 7 + cy] >> (4 - gc)) & 1) {
                                const int t = vis_lane(qe.y, l);
                                c0 = t & 255, c1 = (t >> 8) & 255, c2 = (t >> 16) & 255;
                            }
                        }
                    }
                }
            }
        }
    }

    if (full) {
        const unsigned pix = (unsigned)vis_pack3(c0, c1, c2);
        const int q = min((lane * 4) / 3, 62), sh = (lane * 4 - q * 3) * 8;      // lanes >= 48 shuffle along and store nothing
        const unsigned a = __shfl(pix, q, 64), b = __shfl(pix, q + 1, 64);
        const unsigned d = (unsigned)((((unsigned long long)b << 24) | a) >> sh);
        if (lane < 48) reinterpret_cast<uint32_t*>(out + p0 * 3)[lane] = d;
    } else if (p < HW) {
        out[p * 3] = (uint8_t)c0, out[p * 3 + 1] = (uint8_t)c1, out[p * 3 + 2] = (uint8_t)c2;
    }
}

// a keypoint (x, y, score) -> its integer centre; false when it is not drawn
__device__ inline bool vis_kp_visible(const float* __restrict__ kp, float thr, int& x, int& y) {
    const float fx = kp[0], fy = kp[1], sc = kp[2];
    if (!(sc > thr) || fx != fx || fy != fy) return false;
    x = vis_floor_clamped(fx, 32768.f), y = vis_floor_clamped(fy, 32768.f);
    return true;
}

// grid = n * (S + K) primitives: of the instance at draw position j first its S segments, then its K discs; sequence number prim + 1
__global__ __launch_bounds__(256) void vis_kp_raise_kernel(const float* __restrict__ kps, const int32_t* __restrict__ recs, int K, const int32_t* __restrict__ skel,
                                                          int S, float thr, int lw, int H, int W, int32_t* __restrict__ win) {
    const int prim = blockIdx.x, j = prim / (S + K), t = prim - j * (S + K);
    const float* kp = kps + (long)recs[(long)j * VIS_REC + VR_SRC] * K * 3;
    int ax, ay, bx, by, rad;
    const bool seg = t < S;
    if (seg) {
        const int ka = skel[2 * t], kb = skel[2 * t + 1];
        if (ka < 0 || ka >= K || kb < 0 || kb >= K) return;
        if (!vis_kp_visible(kp + 3 * ka, thr, ax, ay) || !vis_kp_visible(kp + 3 * kb, thr, bx, by)) return;
        rad = lw;                                                    // 4 d^2 <= lw^2: within lw / 2 of the segment
    } else {
        if (!vis_kp_visible(kp + 3 * (t - S), thr, ax, ay)) return;
        bx = ax, by = ay;
        rad = max(2, lw + 1);
    }
    const int x0 = max(min(ax, bx) - rad, 0), x1 = min(max(ax, bx) + rad, W - 1);
    const int y0 = max(min(ay, by) - rad, 0), y1 = min(max(ay, by) + rad, H - 1);
    if (x0 > x1 || y0 > y1) return;
    const long long dx = bx - ax, dy = by - ay, dd = dx * dx + dy * dy, lw2 = (long long)lw * lw;
    // the bounding box in 16 x 16 tiles, a thread per pixel.  A tile whose centre is further from the segment than the primitive's reach
    // plus the tile's half diagonal (11.4) holds no pixel of it: a float test with a pixel to spare skips it for the whole workgroup;
    // which pixels of the other tiles are on is decided by the exact integer test alone.
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const float fdx = (float)dx, fdy = (float)dy, fdd = (float)dd, reach = (float)rad + 13.f;
    for (int ty0 = y0; ty0 <= y1; ty0 += 16) {
        for (int tx0 = x0; tx0 <= x1; tx0 += 16) {
            const float cx = (float)(tx0 - ax) + 7.5f, cy = (float)(ty0 - ay) + 7.5f;
            const float tc = fdd > 0.f ? fminf(fmaxf((cx * fdx + cy * fdy) / fdd, 0.f), 1.f) : 0.f;
            const float ex = cx - tc * fdx, ey = cy - tc * fdy;
            if (ex * ex + ey * ey > reach * reach) continue;         // uniform over the workgroup
            const int xx = tx0 + tx, yy = ty0 + ty;
            if (xx > x1 || yy > y1) continue;
            const long long ux = xx - ax, uy = yy - ay;
            bool on;
            if (!seg) {
                on = ux * ux + uy * uy <= (long long)rad * rad;
            } else {
                const long long tt = ux * dx + uy * dy;
                if (tt <= 0) {
                    on = 4 * (ux * ux + uy * uy) <= lw2;
                } else if (tt >= dd) {
                    const long long vx = xx - bx, vy = yy - by;
                    on = 4 * (vx * vx + vy * vy) <= lw2;
                } else {
                    const long long cr = ux * dy - uy * dx;          // |cr| < 2^34; lw^2 * dd < 2^42, so a |cr| of 2^21 or more is off
                    on = cr > -(1ll << 21) && cr < (1ll << 21) && 4 * cr * cr <= lw2 * dd;
                }
            }
            if (on) atomicMax(win + (long)yy * W + xx, prim + 1);
        }
    }
}

// the winner map starts at "no primitive": a kernel of the library's own, so that a captured draw replays it like every other node
__global__ __launch_bounds__(256) void vis_kp_clear_kernel(int32_t* __restrict__ win, long HW) {
    for (long p = (long)blockIdx.x * 256 + threadIdx.x; p < HW; p += (long)gridDim.x * 256) win[p] = 0;
}

__global__ __launch_bounds__(256) void vis_kp_colour_kernel(uint8_t* __restrict__ image, long HW, const int32_t* __restrict__ win, const int32_t* __restrict__ recs,
                                                           int S, int K, int kp_col) {
    for (long p = (long)blockIdx.x * 256 + threadIdx.x; p < HW; p += (long)gridDim.x * 256) {
        const int v = win[p];
        if (v <= 0) continue;
        const int j = (v - 1) / (S + K), t = (v - 1) - j * (S + K);
        const int c = t < S ? recs[(long)j * VIS_REC + VR_COL] : kp_col;
        image[p * 3] = (uint8_t)(c & 255), image[p * 3 + 1] = (uint8_t)((c >> 8) & 255), image[p * 3 + 2] = (uint8_t)((c >> 16) & 255);
    }
}

// ---- video: the track table ---------------------------------------------------------------------------------------------------------
constexpr int VT_MAX = 1024;         // rows of a track table and new instances of a frame: one thread each in the assign workgroup
constexpr int VT_NONE = 0x7fffffff;  // "no old row claims this instance"
constexpr int VC_TRACKS = 0, VC_NEXT = 1, VC_DROPPED = 2;      // counters

// pycocotools' box IoU on the corners, float64, every operation rounded on its own: the NumPy restatement does the same operations
__device__ inline double vis_box_iou(const float* __restrict__ a, const float* __restrict__ b) {
#pragma clang fp contract(off)
    const double ax1 = a[0], ay1 = a[1], ax2 = a[2], ay2 = a[3], bx1 = b[0], by1 = b[1], bx2 = b[2], by2 = b[3];
    if (ax1 != ax1 || ay1 != ay1 || ax2 != ax2 || ay2 != ay2 || bx1 != bx1 || by1 != by1 || bx2 != bx2 || by2 != by2) return 0.0;
    const double iw = (ax2 < bx2 ? ax2 : bx2) - (ax1 > bx1 ? ax1 : bx1), ih = (ay2 < by2 ? ay2 : by2) - (ay1 > by1 ? ay1 : by1);
    const double inter = (iw > 0.0 && ih > 0.0) ? iw * ih : 0.0;
    const double aa = (ax2 - ax1) * (ay2 - ay1), ab = (bx2 - bx1) * (by2 - by1);
    const double u = aa + ab - inter;
    if (!(u != 0.0)) return 0.0;                                     // a zero union, or a NaN one (inf - inf)
    const double v = inter / u;
    return v != v ? 0.0 : v;
}

// grid = ceil(rows * n / 256)
__global__ __launch_bounds__(256) void vis_track_iou_kernel(const float* __restrict__ old_boxes, int rows, const float* __restrict__ new_boxes, int n,
                                                           double* __restrict__ iou) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= rows * n) return;
    const int i = k / n, j = k - i * n;
    iou[k] = vis_box_iou(old_boxes + 4 * i, new_boxes + 4 * j);
}

// exclusive scan of one flag per thread over the 1024 threads of the assign workgroup; total: how many are set
__device__ inline int vis_scan_flags(bool flag, int* wsum, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long b = __ballot(flag);
    __syncthreads();                                                 // the readers of the scan before this one are done with wsum
    if (lane == 0) wsum[wave] = __popcll(b);
    __syncthreads();
    int before = 0;
    total = 0;
#pragma unroll
    for (int k = 0; k < VT_MAX / 64; ++k) {
        const int s = wsum[k];
        before += k < wave ? s : 0;
        total += s;
    }
    return before + __popcll(b & ((1ull << lane) - 1ull));
}

// grid = 1.  Thread t is new instance t and old row t; wave w walks the old rows w, w + 16, ..
__global__ __launch_bounds__(VT_MAX) void vis_track_assign_kernel(
    const double* __restrict__ iou, const int32_t* __restrict__ inter, const int32_t* __restrict__ old_areas, const int32_t* __restrict__ new_areas, int rows,
    const float* __restrict__ old_boxes, const long long* __restrict__ old_cls, const int32_t* __restrict__ old_ids, const int32_t* __restrict__ old_ttl,
    const float* __restrict__ new_boxes, const long long* __restrict__ new_cls, int n, int cap, int ttl, double thr, float* __restrict__ out_boxes,
    long long* __restrict__ out_cls, int32_t* __restrict__ out_ids, int32_t* __restrict__ out_ttl, int32_t* __restrict__ src,
    int32_t* __restrict__ track_ids, int32_t* counters) {
    __shared__ int claim[VT_MAX], best[VT_MAX], wsum[VT_MAX / 64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int T = min(max(counters[VC_TRACKS], 0), rows);            // rows at or beyond n_tracks are never read as tracks
    const int next_id = counters[VC_NEXT], dropped = counters[VC_DROPPED];
    claim[t] = VT_NONE;
    best[t] = -1;
    __syncthreads();

    for (int i = wave; i < T; i += VT_MAX / 64) {
        const long long ci = old_cls[i];
        double bv = 0.0;
        int bj = VT_NONE;                                            // lanes walk j upwards: a later equal value never replaces an earlier one
        for (int j = lane; j < n; j += 64) {
            double v = 0.0;
            if (new_cls[j] == ci) {
                if (iou) {
                    v = iou[(long)i * n + j];
                } else {
                    const long long in = inter[(long)i * n + j], u = (long long)old_areas[i] + (long long)new_areas[j] - in;
                    v = u != 0 ? (double)in / (double)u : 0.0;
                }
                if (v != v) v = 0.0;
            }
            if (bj == VT_NONE || v > bv) bv = v, bj = j;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {                           // first maximum of the row: the larger value, then the smaller j
            const double ov = __shfl_xor(bv, o, 64);
            const int oj = __shfl_xor(bj, o, 64);
            if (oj != VT_NONE && (bj == VT_NONE || ov > bv || (ov == bv && oj < bj))) bv = ov, bj = oj;
        }
        if (lane == 0 && bj != VT_NONE && bv > thr) {
            best[i] = bj;
            atomicMin(&claim[bj], i);
        }
    }
    __syncthreads();

    // new instances: the claimed ones inherit, the others are numbered in order of j
    const bool is_new = t < n;
    const int owner = is_new ? claim[t] : VT_NONE;
    const bool fresh = is_new && owner == VT_NONE;
    int n_fresh;
    const int rank = vis_scan_flags(fresh, wsum, n_fresh);
    if (is_new) {
        const int id = fresh ? next_id + rank : old_ids[owner];
        track_ids[t] = id;
        out_ids[t] = id, out_ttl[t] = ttl, out_cls[t] = new_cls[t], src[t] = t;
#pragma unroll
        for (int c = 0; c < 4; ++c) out_boxes[4 * t + c] = new_boxes[4 * t + c];
    }

    // old rows: a row that did not hand its id on ages, and survives behind the new instances while it has time to live and a slot
    bool extra = false;
    int left = 0;
    if (t < T) {
        const int b = best[t];
        left = old_ttl[t] - 1;
        extra = !(b >= 0 && claim[b] == t) && left > 0;
    }
    int n_extra;
    const int slot = n + vis_scan_flags(extra, wsum, n_extra);
    if (extra && slot < cap) {
        out_ids[slot] = old_ids[t], out_ttl[slot] = left, out_cls[slot] = old_cls[t], src[slot] = n + t;
#pragma unroll
        for (int c = 0; c < 4; ++c) out_boxes[4 * slot + c] = old_boxes[4 * t + c];
    }
    if (t == 0) {                                                    // every thread read the counters before the first barrier
        const int kept = min(n_extra, cap - n);
        counters[VC_TRACKS] = n + kept;
        counters[VC_NEXT] = next_id + n_fresh;
        counters[VC_DROPPED] = dropped + (n_extra - kept);
    }
}

// grid = (min(ceil(nw / 256), 256), rows): out row s from new instance src[s] or old row src[s] - n
__global__ __launch_bounds__(256) void vis_track_gather_kernel(const int32_t* __restrict__ src, const int32_t* __restrict__ counters,
                                                              const unsigned long long* __restrict__ old_words, const int32_t* __restrict__ old_areas,
                                                              const unsigned long long* __restrict__ new_words, const int32_t* __restrict__ new_areas, int n,
                                                              int cap, int nw, unsigned long long* __restrict__ out_words, int32_t* __restrict__ out_areas) {
    const int s = blockIdx.y;
    if (s >= min(counters[VC_TRACKS], cap)) return;
    const int v = src[s];
    const unsigned long long* from;
    int area;
    if (v >= 0 && v < n) {
        from = new_words + (long)v * nw, area = new_areas[v];
    } else if (v >= n && v - n < cap) {
        from = old_words + (long)(v - n) * nw, area = old_areas[v - n];
    } else {
        return;                                                      // never read outside the tables, whatever src holds
    }
    unsigned long long* to = out_words + (long)s * nw;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < nw; i += gridDim.x * 256) to[i] = from[i];
    if (blockIdx.x == 0 && threadIdx.x == 0) out_areas[s] = area;
}

// shared argument check of the track entries
inline int vis_track_check(const char* what, int n, int rows, int max_tracks) {
    if (max_tracks < 1 || max_tracks > VT_MAX) return fail(CMK_EINVAL, "%s: max_tracks = %ld outside [1, 1024]", what, max_tracks);
    if (n < 0 || n > max_tracks) return fail(CMK_EINVAL, "%s: %ld instances outside [0, max_tracks = %ld]", what, n, max_tracks);
    if (rows < 0 || rows > max_tracks) return fail(CMK_EINVAL, "%s: %ld rows outside [0, max_tracks = %ld]", what, rows, max_tracks);
    return CMK_OK;
}

inline bool vis_overlap(const void* a, int64_t abytes, const void* b, int64_t bbytes) {
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa < pb + (uintptr_t)bbytes && pb < pa + (uintptr_t)abytes;
}

// shared argument check; the messages name the entry
inline int vis_check(const char* what, int H, int W, int n) {
    if (H < 1 || W < 1) return fail(CMK_EINVAL, "%s: H = %ld, W = %ld must be at least 1", what, H, W);
    if ((int64_t)H * W >= 0x7fffffffLL) return fail(CMK_EINVAL, "%s: H*W of %ld x %ld does not leave int32 pixel positions", what, H, W);
    if (n < 0 || n > 65535) return fail(CMK_EINVAL, "%s: instance count %ld outside [0, 65535]", what, n);
    return CMK_OK;
}

inline int vis_check_width(const char* what, const char* name, int v) {
    if (v >= 1 && v <= 16) return CMK_OK;
    snprintf(g_err, sizeof(g_err), "%s: %s = %d outside [1, 16]", what, name, v);
    return CMK_EINVAL;
}

// ---- contours: exact outlines of the packed masks ---------------------------------------------------------------------------------
// A lattice row y in [0, H] of a mask is LW = ceil((W + 1) / 64) words of 64 vertices; entry e = y * LW + k is word k of row y, NE =
// (H + 1) * LW entries per mask.  Of the 2x2 pixels around vertex (x, y), bit x - 64 k of ne/nwb is pixel (y - 1, x) / (y - 1, x - 1), of
// se/sw pixel (y, x) / (y, x - 1).  A vertex with one or three of them set is a corner (one record), one with the two diagonal ones set a
// saddle (two records).  Records are numbered in lattice row-major order, the two of a saddle with the pass whose horizontal edge lies to
// the left first: the corners of a lattice row then pair up (2m, 2m + 1) into its horizontal segments, and the number of a record is its
// canonical (y, x) rank.  Directions: 0 +x, 1 +y, 2 -x, 3 -y (y down, foreground on the right).
constexpr int VC_BLOCK = 1024;       // records or entries per workgroup of the scans
constexpr long VC_LINK_GRID = 1L << 22;       // workgroups of the link kernel at most: 2^32 threads in x are never reached

// columns x0 .. x0 + 63 of row y as 64 bits; columns outside [0, W) and rows outside [0, H) read as zero
__device__ inline unsigned long long vis_contour_row64(const unsigned long long* __restrict__ w, int nw, int H, int W, int y, long x0) {
    if (y < 0 || y >= H || x0 >= W || x0 <= -64) return 0ull;
    unsigned long long v = vis_bits64(w, (long)y * W + x0, nw);
    if (x0 < 0) v &= ~0ull << (int)(-x0);
    const long n = (long)W - x0;
    if (n < 64) v &= (1ull << n) - 1ull;
    return v;
}

struct VisContourBits {
    unsigned long long ne, nwb, se, sw, corner, saddle;
};

__device__ inline VisContourBits vis_contour_bits(const unsigned long long* __restrict__ w, int nw, int H, int W, int y, int k) {
    VisContourBits b;
    const long x0 = (long)k * 64;
    b.ne = vis_contour_row64(w, nw, H, W, y - 1, x0), b.nwb = vis_contour_row64(w, nw, H, W, y - 1, x0 - 1);
    b.se = vis_contour_row64(w, nw, H, W, y, x0), b.sw = vis_contour_row64(w, nw, H, W, y, x0 - 1);
    b.corner = b.ne ^ b.nwb ^ b.se ^ b.sw;
    b.saddle = (b.ne ^ b.nwb) & (b.se ^ b.sw) & (b.ne ^ b.se);
    return b;
}

// records in front of vertex bit j of an entry
__device__ inline int vis_contour_rank(const VisContourBits& b, int j) {
    const unsigned long long below = (1ull << j) - 1ull;
    return __popcll(b.corner & below) + 2 * __popcll(b.saddle & below);
}

__device__ inline int vis_contour_pix(const unsigned long long* __restrict__ w, int H, int W, int y, int x) {
    if (x < 0 || x >= W || y < 0 || y >= H) return 0;
    const long p = (long)y * W + x;
    return (int)((w[p >> 6] >> (p & 63)) & 1ull);
}

// exclusive scan of one value per thread over the VC_BLOCK threads of a workgroup; total: their sum
__device__ inline long long vis_contour_block_scan(long long v, long long* wsum, long long& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    long long inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const long long t = __shfl_up(inc, o, 64);
        if (lane >= o) inc += t;
    }
    __syncthreads();                                                 // the readers of the scan before this one are done with wsum
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    long long before = 0;
    total = 0;
#pragma unroll
    for (int k = 0; k < VC_BLOCK / 64; ++k) {
        const long long s = wsum[k];
        before += k < wave ? s : 0;
        total += s;
    }
    return before + inc - v;
}

// grid = (NB = ceil(NE / VC_BLOCK), R), one pass over the words: inc[r][e] = records of the entries of e's block up to and with e,
// grp[r][block] = records of the block
__global__ __launch_bounds__(VC_BLOCK) void vis_contour_count_kernel(const unsigned long long* __restrict__ words, int nw, int H, int W, int LW, long NE,
                                                                    int32_t* __restrict__ inc, long long* __restrict__ grp) {
    __shared__ long long wsum[VC_BLOCK / 64];
    const long e = (long)blockIdx.x * VC_BLOCK + threadIdx.x;
    const int r = blockIdx.y;
    long long v = 0;
    if (e < NE) {
        const int y = (int)(e / LW), k = (int)(e - (long)y * LW);
        const VisContourBits b = vis_contour_bits(words + (long)r * nw, nw, H, W, y, k);
        v = __popcll(b.corner) + 2 * __popcll(b.saddle);
    }
    long long total;
    const long long ex = vis_contour_block_scan(v, wsum, total);
    if (e < NE) inc[(long)r * NE + e] = (int32_t)(ex + v);           // at most 128 * VC_BLOCK
    if (threadIdx.x == 0) grp[(long)r * gridDim.x + blockIdx.x] = total;
}

// grid = 1: grp (R * NB block totals, masks in order) -> their exclusive prefix sums in place: the number of the first record of every
// block among the records of all masks; off[r] = that of mask r, off[R] = all, n_corners[r] = off[r + 1] - off[r] (-1 beyond int32)
__global__ __launch_bounds__(VC_BLOCK) void vis_contour_offsets_kernel(long long* __restrict__ grp, int R, int NB, long long* __restrict__ off,
                                                                      int32_t* __restrict__ n_corners) {
    __shared__ long long wsum[VC_BLOCK / 64];
    const long n = (long)R * NB;
    long long carry = 0;
    for (long base = 0; base < n; base += VC_BLOCK) {
        const long g = base + threadIdx.x;
        const long long v = g < n ? grp[g] : 0;
        long long total;
        const long long ex = carry + vis_contour_block_scan(v, wsum, total);
        if (g < n) grp[g] = ex;
        carry += total;
    }
    __syncthreads();                                                 // the prefix sums are in memory for every thread of the workgroup
    for (int r = threadIdx.x; r < R; r += VC_BLOCK) {
        const long long a = grp[(long)r * NB], b = r + 1 < R ? grp[(long)(r + 1) * NB] : carry;
        off[r] = a;
        n_corners[r] = b - a > 0x7fffffffLL ? -1 : (int32_t)(b - a);
    }
    if (threadIdx.x == 0) off[R] = carry;
}

// the number of the first record of entry e among the records of all masks; count: the records of the entry
__device__ inline long long vis_contour_first(const int32_t* __restrict__ inc, const long long* __restrict__ grp, long e, int& count) {
    const int here = inc[e], prev = (e & (VC_BLOCK - 1)) ? inc[e - 1] : 0;
    count = here - prev;
    return grp[e / VC_BLOCK] + prev;
}

// grid = (ceil(NE / 256), R), a thread per entry; an entry without a corner reads two counts and no row.  rec[i] = (x, y, out direction,
// mask) for the corners of the entry in order of x, at most 64 trips
__global__ __launch_bounds__(256) void vis_contour_emit_kernel(const unsigned long long* __restrict__ words, int nw, int H, int W, int LW, long NE,
                                                              int NB, const int32_t* __restrict__ inc, const long long* __restrict__ grp, int T,
                                                              int4* __restrict__ rec) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= NE) return;
    const int r = blockIdx.y;
    int count;
    long long i = vis_contour_first(inc + (long)r * NE, grp + (long)r * NB, e, count);
    if (count <= 0) return;
    const int y = (int)(e / LW), k = (int)(e - (long)y * LW);
    const VisContourBits b = vis_contour_bits(words + (long)r * nw, nw, H, W, y, k);
    unsigned long long any = b.corner | b.saddle;
    for (int t = 0; t < 64 && any; ++t) {
        const int j = __builtin_ctzll(any);
        any &= any - 1ull;
        const bool sad = (b.saddle >> j) & 1ull;
        if (i < 0 || i + (sad ? 1 : 0) >= (long long)T) return;      // never outside the T records the host sized, whatever ws holds
        const int NWp = (int)((b.nwb >> j) & 1ull), NEp = (int)((b.ne >> j) & 1ull), SWp = (int)((b.sw >> j) & 1ull), SEp = (int)((b.se >> j) & 1ull);
        const int x = k * 64 + j;
        if (sad) {
            rec[i] = make_int4(x, y, NWp ? 2 : 1, r);
            rec[i + 1] = make_int4(x, y, NWp ? 0 : 3, r);
            i += 2;
        } else {
            rec[i] = make_int4(x, y, (SEp && !NEp) ? 0 : ((SWp && !SEp) ? 1 : ((NWp && !SWp) ? 2 : 3)), r);
            i += 1;
        }
    }
}

// one record of the link kernel, by one wave: everything is wave-uniform but the row a lane tests
__device__ inline void vis_contour_link_one(const unsigned long long* __restrict__ words, int nw, int R, int H, int W, int LW, long NE, int NB,
                                            const int32_t* __restrict__ inc, const long long* __restrict__ grp, int T, const int4* __restrict__ rec,
                                            int32_t* __restrict__ succ, long i, int lane) {
    const int4 q = rec[i];
    const int x = q.x, y = q.y, d = q.z, r = q.w;
    long long s = i;
    if (r >= 0 && r < R && x >= 0 && x <= W && y >= 0 && y <= H) {   // a record nobody wrote links to itself and reads nothing
        if (d == 0 || d == 2) {
            s = i ^ 1;
        } else if (d == 1 || d == 3) {
            const unsigned long long* w = words + (long)r * nw;
            int yy = d == 1 ? H : 0;
            const int trips = cdiv(H, 64) + 1;
            for (int t = 0; t < trips; ++t) {
                bool stop;
                int cand;
                if (d == 1) {                                        // down while the row below the vertex still has (set, unset)
                    cand = y + 1 + t * 64 + lane;
                    stop = cand >= H || !(vis_contour_pix(w, H, W, cand, x - 1) && !vis_contour_pix(w, H, W, cand, x));
                } else {                                             // up while the row above the vertex still has (unset, set)
                    cand = y - 1 - t * 64 - lane;
                    stop = cand <= 0 || !(!vis_contour_pix(w, H, W, cand - 1, x - 1) && vis_contour_pix(w, H, W, cand - 1, x));
                }
                const unsigned long long hit = __ballot(stop);
                if (hit) {
                    yy = __shfl(cand, __builtin_ctzll(hit), 64);
                    break;
                }
            }
            yy = min(max(yy, 0), H);
            const int k = x >> 6, j = x & 63;
            const VisContourBits b = vis_contour_bits(w, nw, H, W, yy, k);
            int count;
            s = vis_contour_first(inc + (long)r * NE, grp + (long)r * NB, (long)yy * LW + k, count) + vis_contour_rank(b, j) +
                ((((b.saddle >> j) & 1ull) && d == 3) ? 1 : 0);
        }
    }
    if (lane == 0) succ[i] = (s < 0 || s >= (long long)T) ? (int32_t)i : (int32_t)s;
}

// grid = min(ceil(T / 4), VC_LINK_GRID), a wave per record, striding: succ[i] = the record the out edge of record i ends at.  A
// horizontal edge ends at record i ^ 1.  A vertical one is followed along its column to the next corner, 64 lattice rows per trip (lane = row, the first lane whose row ends
// the edge wins the ballot), at most ceil(H / 64) + 1 trips; that corner's number is the first of its entry + its rank (+ 1 for the pass
// of a saddle that arrives going up: the walk turns right).
__global__ __launch_bounds__(256) void vis_contour_link_kernel(const unsigned long long* __restrict__ words, int nw, int R, int H, int W, int LW, long NE,
                                                              int NB, const int32_t* __restrict__ inc, const long long* __restrict__ grp, int T,
                                                              const int4* __restrict__ rec, int32_t* __restrict__ succ) {
    const int lane = threadIdx.x & 63;
    for (long i = (long)blockIdx.x * 4 + (threadIdx.x >> 6); i < T; i += (long)gridDim.x * 4)       // wave-uniform
        vis_contour_link_one(words, nw, R, H, W, LW, NE, NB, inc, grp, T, rec, succ, i, lane);
}

// grid = ceil(T / 256), round k of the pointer jumping with hop = 2^k: lab[i] = the smallest record number among the 2 hop records from i
// along the loop, dist[i] = the steps from i to its first occurrence, s[i] = the record 2 hop steps on.  first: lab = i, dist = 0.
__global__ __launch_bounds__(256) void vis_contour_jump_kernel(const int32_t* __restrict__ s_in, const int32_t* __restrict__ lab_in,
                                                              const int32_t* __restrict__ dist_in, int32_t* __restrict__ s_out,
                                                              int32_t* __restrict__ lab_out, int32_t* __restrict__ dist_out, int T, int hop, int first) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= T) return;
    int j = s_in[i];
    if (j < 0 || j >= T) j = (int)i;
    int li = first ? (int)i : lab_in[i], di = first ? 0 : dist_in[i];
    const int lj = first ? j : lab_in[j], dj = first ? 0 : dist_in[j];
    if (lj < li) li = lj, di = hop + dj;                             // an equal label is the same record met again: the earlier one stays
    int sj = s_in[j];
    if (sj < 0 || sj >= T) sj = j;
    s_out[i] = sj, lab_out[i] = li, dist_out[i] = di;
}

// the vertices of the loop that starts at record i, 0 for a record that starts none
__device__ inline int vis_contour_loop_len(const int32_t* __restrict__ succ, const int32_t* __restrict__ lab, const int32_t* __restrict__ dist, int T,
                                           long i) {
    if (i >= T || lab[i] != (int)i) return 0;
    const int s = succ[i];
    return s >= 0 && s < T ? 1 + dist[s] : 1;
}

// grid = ceil(T / VC_BLOCK): bsum[b] = vertices of the loops that start in block b
__global__ __launch_bounds__(VC_BLOCK) void vis_contour_lens_kernel(const int32_t* __restrict__ succ, const int32_t* __restrict__ lab,
                                                                   const int32_t* __restrict__ dist, int T, int32_t* __restrict__ bsum) {
    __shared__ long long wsum[VC_BLOCK / 64];
    const long i = (long)blockIdx.x * VC_BLOCK + threadIdx.x;
    long long total;
    vis_contour_block_scan(vis_contour_loop_len(succ, lab, dist, T, i), wsum, total);
    if (threadIdx.x == 0) bsum[blockIdx.x] = (int32_t)(total > 0x7fffffffLL ? 0x7fffffffLL : total);
}

// grid = 1: bsum -> its exclusive prefix sums in place
__global__ __launch_bounds__(VC_BLOCK) void vis_contour_blocks_kernel(int32_t* __restrict__ bsum, int nb) {
    __shared__ long long wsum[VC_BLOCK / 64];
    long long carry = 0;
    for (int base = 0; base < nb; base += VC_BLOCK) {
        const int b = base + threadIdx.x;
        const long long v = b < nb ? bsum[b] : 0;
        long long total;
        const long long ex = carry + vis_contour_block_scan(v, wsum, total);
        if (b < nb) bsum[b] = (int32_t)(ex > 0x7fffffffLL ? 0x7fffffffLL : ex);
        carry += total;
    }
}

// grid = ceil(T / VC_BLOCK): lo[i] = the output position of the loop that starts at record i: the vertices of all loops that start earlier
__global__ __launch_bounds__(VC_BLOCK) void vis_contour_place_kernel(const int32_t* __restrict__ succ, const int32_t* __restrict__ lab,
                                                                    const int32_t* __restrict__ dist, int T, const int32_t* __restrict__ bsum,
                                                                    int32_t* __restrict__ lo) {
    __shared__ long long wsum[VC_BLOCK / 64];
    const long i = (long)blockIdx.x * VC_BLOCK + threadIdx.x;
    long long total;
    const long long ex = bsum[blockIdx.x] + vis_contour_block_scan(vis_contour_loop_len(succ, lab, dist, T, i), wsum, total);
    if (i < T) lo[i] = (int32_t)(ex > 0x7fffffffLL ? 0x7fffffffLL : ex);
}

// grid = ceil(T / 256): record i goes to the position of its loop + its rank in the walk from the loop's start
__global__ __launch_bounds__(256) void vis_contour_write_kernel(const int4* __restrict__ rec, const int32_t* __restrict__ succ,
                                                               const int32_t* __restrict__ lab, const int32_t* __restrict__ dist,
                                                               const int32_t* __restrict__ lo, int T, int32_t* __restrict__ xy,
                                                               int32_t* __restrict__ head) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= T) return;
    int l = lab[i];
    if (l < 0 || l >= T) l = (int)i;
    const int d = dist[i];
    const int len = vis_contour_loop_len(succ, lab, dist, T, l);
    const long long pos = (long long)lo[l] + (d == 0 ? 0 : len - d);
    if (pos < 0 || pos >= (long long)T) return;
    const int4 q = rec[i];
    xy[2 * pos] = q.x, xy[2 * pos + 1] = q.y;
    head[pos] = d == 0 ? 1 : 0;
}

inline long vis_contour_lw(int W) { return ((long)W + 1 + 63) / 64; }
inline long vis_contour_entries(int H, int W) { return ((long)H + 1) * vis_contour_lw(W); }
inline long vis_contour_groups(int H, int W) { return (vis_contour_entries(H, W) + VC_BLOCK - 1) / VC_BLOCK; }
// [off R + 1 int64 | grp R * NB int64 | inc R * NE int32]
inline int64_t vis_contour_ws_bytes(int R, int H, int W) {
    return 8 * ((int64_t)R + 1) + 8 * (int64_t)R * vis_contour_groups(H, W) + 4 * (int64_t)R * vis_contour_entries(H, W);
}
inline int64_t vis_contour_blocks(int64_t T) { return (T + VC_BLOCK - 1) / VC_BLOCK; }
// [rec 16 T | succ, 2 x (s, lab, dist), lo: 8 x 4 T | bsum 4 nb]
inline int64_t vis_contour_trace_bytes(int64_t T) { return T <= 0 ? 0 : 48 * T + 4 * vis_contour_blocks(T); }

// shared argument check of the two phases; the messages name the entry
inline int vis_contour_check(const char* what, int R, int H, int W, const void* ws, int64_t ws_bytes, bool any_null) {
    if (int rc = vis_check(what, H, W, R)) return rc;
    if (any_null) return fail(CMK_EINVAL, "%s: null pointer", what);
    if ((uintptr_t)ws & 7) return fail(CMK_EINVAL, "%s: workspace is not 8-byte aligned", what);
    if (ws_bytes < vis_contour_ws_bytes(R, H, W))
        return fail(CMK_EINVAL, "%s: workspace of %ld bytes, need %ld", what, (long)ws_bytes, (long)vis_contour_ws_bytes(R, H, W));
    return CMK_OK;
}

}  // namespace cmk

using namespace cmk;

extern "C" int cmk_vis_record_ints(void) { return VIS_REC; }

// cmk_vis_prepare (color_ids null) and cmk_vis_prepare_ids
static int vis_prepare_launch(const char* what, const float* boxes, const float* scores, const int64_t* classes, const int64_t* order,
                              const uint8_t* names, const int32_t* name_lens, int num_names, const uint8_t* palette, int n, int H, int W, int font_scale,
                              int color_by_class, const int32_t* color_ids, int32_t* records, void* stream) {
    if (int rc = vis_check(what, H, W, n)) return rc;
    if (int rc = vis_check_width(what, "font_scale", font_scale)) return rc;
    if (num_names < 0 || num_names > 65535) return fail(CMK_EINVAL, "%s: %ld names outside [0, 65535]", what, num_names);
    if (n == 0) return CMK_OK;
    if (!boxes || !scores || !classes || !order || !palette || !records || (num_names && (!names || !name_lens)))
        return fail(CMK_EINVAL, "%s: null pointer", what);
    hipLaunchKernelGGL(vis_prepare_kernel, dim3(cdiv(n, 64)), dim3(64), 0, (hipStream_t)stream, boxes, scores, (const long long*)classes,
                       (const long long*)order, names, name_lens, num_names, palette, n, H, W, font_scale, color_by_class ? 1 : 0, color_ids, records);
    return check_launch(what);
}

extern "C" int cmk_vis_prepare(const float* boxes, const float* scores, const int64_t* classes, const int64_t* order, const uint8_t* names,
                               const int32_t* name_lens, int num_names, const uint8_t* palette, int n, int H, int W, int font_scale, int color_by_class,
                               int32_t* records, void* stream) {
    return vis_prepare_launch("vis_prepare", boxes, scores, classes, order, names, name_lens, num_names, palette, n, H, W, font_scale, color_by_class,
                              nullptr, records, stream);
}

extern "C" int cmk_vis_prepare_ids(const float* boxes, const float* scores, const int64_t* classes, const int64_t* order, const uint8_t* names,
                                   const int32_t* name_lens, int num_names, const uint8_t* palette, int n, int H, int W, int font_scale,
                                   int color_by_class, const int32_t* color_ids, int32_t* records, void* stream) {
    return vis_prepare_launch("vis_prepare_ids", boxes, scores, classes, order, names, name_lens, num_names, palette, n, H, W, font_scale,
                              color_by_class, color_ids, records, stream);
}

extern "C" int cmk_vis_track_iou_boxes(const float* old_boxes, int rows, const float* new_boxes, int n, double* iou, void* stream) {
    if (int rc = vis_track_check("vis_track_iou_boxes", n, rows, VT_MAX)) return rc;
    if (rows == 0 || n == 0) return CMK_OK;
    if (!old_boxes || !new_boxes || !iou) return fail(CMK_EINVAL, "%s: null pointer", "vis_track_iou_boxes");
    hipLaunchKernelGGL(vis_track_iou_kernel, dim3(cdiv(rows * n, 256)), dim3(256), 0, (hipStream_t)stream, old_boxes, rows, new_boxes, n, iou);
    return check_launch("vis_track_iou_boxes");
}

extern "C" int cmk_vis_track_assign(const double* iou, const int32_t* inter, const int32_t* old_areas, const int32_t* new_areas, int rows,
                                    const float* old_boxes, const int64_t* old_classes, const int32_t* old_ids, const int32_t* old_ttl,
                                    const float* new_boxes, const int64_t* new_classes, int n, int max_tracks, int ttl, double threshold,
                                    float* out_boxes, int64_t* out_classes, int32_t* out_ids, int32_t* out_ttl, int32_t* src, int32_t* track_ids,
                                    int32_t* counters, void* stream) {
    const char* what = "vis_track_assign";
    if (int rc = vis_track_check(what, n, rows, max_tracks)) return rc;
    if (ttl < 1 || ttl > 255) return fail(CMK_EINVAL, "%s: ttl = %ld outside [1, 255]", what, ttl);
    if (!(threshold >= 0.0 && threshold <= 1.0)) return fail(CMK_EINVAL, "%s: the IoU threshold is outside [0, 1]", what);
    if (!old_boxes || !old_classes || !old_ids || !old_ttl || !out_boxes || !out_classes || !out_ids || !out_ttl || !src || !counters ||
        (n && (!new_boxes || !new_classes || !track_ids)))
        return fail(CMK_EINVAL, "%s: null pointer", what);
    if (n && rows) {
        if ((iou != nullptr) == (inter != nullptr)) return fail(CMK_EINVAL, "%s: exactly one of the iou and inter tables must be given", what);
        if (inter && (!old_areas || !new_areas)) return fail(CMK_EINVAL, "%s: null pointer (the inter table needs both area arrays)", what);
    }
    const int64_t cap = max_tracks;                                  // a thread reads old row t after another wrote out row t: byte ranges, not pointers
    if (vis_overlap(out_boxes, 16 * cap, old_boxes, 16 * cap) || vis_overlap(out_classes, 8 * cap, old_classes, 8 * cap) ||
        vis_overlap(out_ids, 4 * cap, old_ids, 4 * cap) || vis_overlap(out_ttl, 4 * cap, old_ttl, 4 * cap))
        return fail(CMK_EINVAL, "%s: the new table overlaps the old one; the update is out of place", what);
    hipLaunchKernelGGL(vis_track_assign_kernel, dim3(1), dim3(VT_MAX), 0, (hipStream_t)stream, (n && rows) ? iou : nullptr, inter, old_areas, new_areas,
                       rows, old_boxes, (const long long*)old_classes, old_ids, old_ttl, new_boxes, (const long long*)new_classes, n, max_tracks, ttl,
                       threshold, out_boxes, (long long*)out_classes, out_ids, out_ttl, src, track_ids, counters);
    return check_launch(what);
}

extern "C" int cmk_vis_track_gather(const int32_t* src, const int32_t* counters, const uint64_t* old_words, const int32_t* old_areas,
                                    const uint64_t* new_words, const int32_t* new_areas, int n, int rows, int max_tracks, int H, int W,
                                    uint64_t* out_words, int32_t* out_areas, void* stream) {
    const char* what = "vis_track_gather";
    if (int rc = vis_check(what, H, W, 0)) return rc;
    if (int rc = vis_track_check(what, n, rows, max_tracks)) return rc;
    if (!src || !counters || !old_words || !old_areas || !out_words || !out_areas || (n && (!new_words || !new_areas)))
        return fail(CMK_EINVAL, "%s: null pointer", what);
    const int nw = (int)(((int64_t)H * W + 63) / 64);
    const int64_t row = (int64_t)nw * 8;
    if (vis_overlap(out_words, row * max_tracks, old_words, row * max_tracks) || (n && vis_overlap(out_words, row * max_tracks, new_words, row * n)) ||
        vis_overlap(out_areas, 4 * (int64_t)max_tracks, old_areas, 4 * (int64_t)max_tracks))
        return fail(CMK_EINVAL, "%s: the new table overlaps the old one or the new instances; the gather is out of place", what);
    if (rows == 0) return CMK_OK;
    hipLaunchKernelGGL(vis_track_gather_kernel, dim3(min(cdiv(nw, 256), 256), rows), dim3(256), 0, (hipStream_t)stream, src, counters,
                       (const unsigned long long*)old_words, old_areas, (const unsigned long long*)new_words, new_areas, n, max_tracks, nw,
                       (unsigned long long*)out_words, out_areas);
    return check_launch(what);
}

extern "C" int cmk_vis_compose(const uint8_t* image_in, uint8_t* image_out, int H, int W, const uint64_t* words, const int32_t* records, int n,
                               const uint8_t* font, int line_width, int font_scale, int alpha256, void* stream) {
    if (int rc = vis_check("vis_compose", H, W, n)) return rc;
    if (int rc = vis_check_width("vis_compose", "line_width", line_width)) return rc;
    if (int rc = vis_check_width("vis_compose", "font_scale", font_scale)) return rc;
    if (alpha256 < 0 || alpha256 > 256) return fail(CMK_EINVAL, "%s: alpha256 = %ld outside [0, 256]", "vis_compose", alpha256);
    if (!image_in || !image_out || (n && (!records || !font))) return fail(CMK_EINVAL, "%s: null pointer", "vis_compose");
    const int64_t bytes = (int64_t)H * W * 3;
    if (image_in < image_out + bytes && image_out < image_in + bytes)
        return fail(CMK_EINVAL, "%s: image_out overlaps image_in; the compose pass is out of place", "vis_compose");
    if ((uintptr_t)records & 15) return fail(CMK_EINVAL, "%s: records must be 16-byte aligned", "vis_compose");
    const int nw = (int)(((int64_t)H * W + 63) / 64);
    const int vec = (((uintptr_t)image_in | (uintptr_t)image_out) & 3) == 0;
    hipLaunchKernelGGL(vis_compose_kernel, dim3(cdiv(nw, 4)), dim3(256), 0, (hipStream_t)stream, image_in, image_out, H, W, nw,
                       (const unsigned long long*)words, records, n, font, line_width, font_scale, alpha256, vec);
    return check_launch("vis_compose");
}

extern "C" int cmk_vis_keypoints(uint8_t* image, int H, int W, const float* keypoints, const int32_t* records, int n, int num_keypoints,
                                 const int32_t* skeleton, int num_segments, float threshold, int line_width, int keypoint_color, int32_t* winner,
                                 void* stream) {
    if (int rc = vis_check("vis_keypoints", H, W, n)) return rc;
    if (int rc = vis_check_width("vis_keypoints", "line_width", line_width)) return rc;
    if (num_keypoints < 1 || num_keypoints > 1024) return fail(CMK_EINVAL, "%s: %ld keypoints outside [1, 1024]", "vis_keypoints", num_keypoints);
    if (num_segments < 0 || num_segments > 4096) return fail(CMK_EINVAL, "%s: %ld skeleton segments outside [0, 4096]", "vis_keypoints", num_segments);
    if (n == 0) return CMK_OK;
    if (!image || !keypoints || !records || !winner || (num_segments && !skeleton)) return fail(CMK_EINVAL, "%s: null pointer", "vis_keypoints");
    hipStream_t st = (hipStream_t)stream;
    const int64_t HW = (int64_t)H * W;
    hipLaunchKernelGGL(vis_kp_clear_kernel, dim3(stream_grid(HW)), dim3(256), 0, st, winner, (long)HW);
    hipLaunchKernelGGL(vis_kp_raise_kernel, dim3(n * (num_segments + num_keypoints)), dim3(256), 0, st, keypoints, records, num_keypoints, skeleton,
                       num_segments, threshold, line_width, H, W, winner);
    hipLaunchKernelGGL(vis_kp_colour_kernel, dim3(stream_grid(HW)), dim3(256), 0, st, image, (long)HW, (const int32_t*)winner, records, num_segments,
                       num_keypoints, keypoint_color);
    return check_launch("vis_keypoints");
}

extern "C" int64_t cmk_vis_contour_ws_bytes(int R, int H, int W) {
    if (R < 0 || R > 65535 || H < 1 || W < 1 || (int64_t)H * W >= 0x7fffffffLL) return 0;
    return vis_contour_ws_bytes(R, H, W);
}

extern "C" int64_t cmk_vis_contour_trace_ws_bytes(int total) { return vis_contour_trace_bytes(total); }

extern "C" int cmk_vis_contour_count(const uint64_t* words, int R, int H, int W, void* ws, int64_t ws_bytes, int32_t* n_corners, void* stream) {
    const char* what = "vis_contour_count";
    if (R == 0) return CMK_OK;
    if (int rc = vis_contour_check(what, R, H, W, ws, ws_bytes, !words || !ws || !n_corners)) return rc;
    const int nw = (int)(((int64_t)H * W + 63) / 64);
    const int64_t in_bytes = (int64_t)R * nw * 8, need = vis_contour_ws_bytes(R, H, W);
    if (vis_overlap(ws, need, words, in_bytes) || vis_overlap(n_corners, 4 * (int64_t)R, words, in_bytes) ||
        vis_overlap(n_corners, 4 * (int64_t)R, ws, need))
        return fail(CMK_EINVAL, "%s: the workspace or n_corners overlaps the words or each other", what);
    hipStream_t st = (hipStream_t)stream;
    const int LW = (int)vis_contour_lw(W), NB = (int)vis_contour_groups(H, W);
    const long NE = vis_contour_entries(H, W);
    long long* off = (long long*)ws;
    long long* grp = off + R + 1;
    int32_t* inc = (int32_t*)(grp + (long)R * NB);
    hipLaunchKernelGGL(vis_contour_count_kernel, dim3(NB, R), dim3(VC_BLOCK), 0, st, (const unsigned long long*)words, nw, H, W, LW, NE, inc, grp);
    hipLaunchKernelGGL(vis_contour_offsets_kernel, dim3(1), dim3(VC_BLOCK), 0, st, grp, R, NB, off, n_corners);
    return check_launch(what);
}

extern "C" int cmk_vis_contour_trace(const uint64_t* words, int R, int H, int W, const void* ws, int64_t ws_bytes, const int32_t* n_corners,
                                     void* scratch, int64_t scratch_bytes, int32_t* xy, int32_t* head, void* stream) {
    const char* what = "vis_contour_trace";
    if (R == 0) return CMK_OK;
    if (int rc = vis_contour_check(what, R, H, W, ws, ws_bytes, !words || !ws || !n_corners)) return rc;
    int64_t T = 0;
    int32_t longest = 0;
    for (int r = 0; r < R; ++r) {
        const int32_t n = n_corners[r];                              // host memory: the totals the caller read back
        if (n < 0 || (n & 1)) return fail(CMK_EINVAL, "%s: n_corners[%ld] = %ld is negative or odd", what, r, n);
        T += n;
        longest = n > longest ? n : longest;
    }
    if (T > 0x7fffffffLL) return fail(CMK_EINVAL, "%s: the corners of all masks, %ld, do not fit int32", what, (long)T);
    if (T == 0) return CMK_OK;
    if (!scratch || !xy || !head) return fail(CMK_EINVAL, "%s: null pointer", what);
    if ((uintptr_t)scratch & 15) return fail(CMK_EINVAL, "%s: scratch is not 16-byte aligned", what);
    if (scratch_bytes < vis_contour_trace_bytes(T))
        return fail(CMK_EINVAL, "%s: scratch of %ld bytes, need %ld", what, (long)scratch_bytes, (long)vis_contour_trace_bytes(T));
    const int nw = (int)(((int64_t)H * W + 63) / 64);
    const int64_t in_bytes = (int64_t)R * nw * 8, ws_need = vis_contour_ws_bytes(R, H, W), sc_need = vis_contour_trace_bytes(T);
    const void* outs[3] = {xy, head, scratch};
    const int64_t out_bytes[3] = {8 * T, 4 * T, sc_need};
    for (int a = 0; a < 3; ++a) {
        if (vis_overlap(outs[a], out_bytes[a], words, in_bytes) || vis_overlap(outs[a], out_bytes[a], ws, ws_need))
            return fail(CMK_EINVAL, "%s: xy, head or scratch overlaps the words or the workspace; the trace is out of place", what);
        for (int b = a + 1; b < 3; ++b)
            if (vis_overlap(outs[a], out_bytes[a], outs[b], out_bytes[b])) return fail(CMK_EINVAL, "%s: xy, head and scratch overlap each other", what);
    }
    hipStream_t st = (hipStream_t)stream;
    const int LW = (int)vis_contour_lw(W), NB = (int)vis_contour_groups(H, W);
    const long NE = vis_contour_entries(H, W);
    const long long* grp = (const long long*)ws + R + 1;
    const int32_t* inc = (const int32_t*)(grp + (long)R * NB);
    const int Ti = (int)T, nb = (int)vis_contour_blocks(T);
    int4* rec = (int4*)scratch;
    int32_t* succ = (int32_t*)(rec + T);
    int32_t* buf[2][3] = {{succ + T, succ + 2 * T, succ + 3 * T}, {succ + 4 * T, succ + 5 * T, succ + 6 * T}};
    int32_t* lo = succ + 7 * T;
    int32_t* bsum = succ + 8 * T;
    const dim3 per_record((unsigned)((T + 255) / 256));
    const unsigned long long* w = (const unsigned long long*)words;
    hipLaunchKernelGGL(vis_contour_emit_kernel, dim3((unsigned)((NE + 255) / 256), R), dim3(256), 0, st, w, nw, H, W, LW, NE, NB, inc, grp, Ti, rec);
    const int64_t link_grid = (T + 3) / 4 < VC_LINK_GRID ? (T + 3) / 4 : VC_LINK_GRID;
    hipLaunchKernelGGL(vis_contour_link_kernel, dim3((unsigned)link_grid), dim3(256), 0, st, w, nw, R, H, W, LW, NE, NB, inc, grp, Ti,
                       (const int4*)rec, succ);
    // after round k a record has seen 2^(k+1) records of its loop, and no loop is longer than the corners of its mask
    int cur = 0;
    for (int k = 0; (1LL << k) < longest; ++k) {
        const int32_t* const* in = k ? buf[cur ^ 1] : nullptr;
        hipLaunchKernelGGL(vis_contour_jump_kernel, per_record, dim3(256), 0, st, k ? in[0] : (const int32_t*)succ, k ? in[1] : nullptr,
                           k ? in[2] : nullptr, buf[cur][0], buf[cur][1], buf[cur][2], Ti, (int)(1LL << k), k ? 0 : 1);
        cur ^= 1;
    }
    const int32_t* lab = buf[cur ^ 1][1];
    const int32_t* dist = buf[cur ^ 1][2];
    hipLaunchKernelGGL(vis_contour_lens_kernel, dim3(nb), dim3(VC_BLOCK), 0, st, (const int32_t*)succ, lab, dist, Ti, bsum);
    hipLaunchKernelGGL(vis_contour_blocks_kernel, dim3(1), dim3(VC_BLOCK), 0, st, bsum, nb);
    hipLaunchKernelGGL(vis_contour_place_kernel, dim3(nb), dim3(VC_BLOCK), 0, st, (const int32_t*)succ, lab, dist, Ti, (const int32_t*)bsum, lo);
    hipLaunchKernelGGL(vis_contour_write_kernel, per_record, dim3(256), 0, st, (const int4*)rec, (const int32_t*)succ, lab, dist, (const int32_t*)lo,
                       Ti, xy, head);
    return check_launch(what);
}
