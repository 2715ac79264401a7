// qs_render.h -- headless software rasteriser: draws selected envs as uint8 RGB frames from the state buffers the
// step kernels keep in HBM (qs_render, include/quadswarm.h).  Read-only on the simulation; one kernel, no host data.
//
// The picture (DESIGN.md "Rendering"; tests/render_restatement.py restates it in numpy):
//   orthographic, one frame [H, W, 3] per selected env, row 0 on top.  View (u, v): topdown (x, y), side (x, z),
//   front (y, z).  Window: the room rectangle on (u, v), or with `follow` the square around the drones' mean with side
//   max(2 max_i |p_i - mean|_inf + 2 m, 2 m).  s = min((W - 8) / span_u, (H - 8) / span_v) px/m;
//   X(u) = W/2 + (u - c_u) s, Y(v) = H/2 - (v - c_v) s; pixel (col, row) is sampled once at (col + .5, row + .5).
//   Layers, later over earlier: background (outside / inside the room), active pillars, flavor-A target (cross of two
//   3 px arms, in topdown also the capture ring), flavor-B goal rings, drones in index order (4 arms, 2 rear rotors in
//   half intensity, 2 front rotors, body), room border.  Arms and cross arms: pixels within QS_RD_SEG_HW of the segment.
//   Rings: r_out - 1 <= d <= r_out.  Border: pixels within QS_RD_BORDER_HW of the room rectangle's outline -- half a
//   pixel plus 2^-10: the 4 px margin puts the room's outline of the limiting axis on whole pixel coordinates, where
//   every pixel centre beside it is exactly half a pixel away; the 2^-10 takes those centres off the knife edge (both
//   neighbouring lines are border there, in every arithmetic).
//
// Kernel shape: grid = (pixel tiles of 64 x 16, selected envs), workgroup = 256 lanes = 4 waves, wave w owns rows
// 4 w .. 4 w + 3 of the tile (lane = column).  Stage 1: the workgroup builds the env's screen-space primitives in LDS
// (drone i on lane i: coalesced loads of the field-major state; computed slots, layer order).  Stage 2: each wave
// compacts the primitives whose bounding box meets its 64 x 4 pixel rectangle into its own index list, in layer
// order (ballot + mbcnt prefix, 64 primitives per pass).  Stage 3: each lane shades its 4 pixels from that list;
// the colours go through LDS and leave as whole dwords, 192 contiguous bytes per row (W % 4 == 0).
#pragma once
#include "qs_common.h"

namespace qs {

// ---- palette: 16 drone colours, their half-intensity variants, the fixed colours (quadswarm_amd.render.PALETTE
// mirrors this table; tests/test_render_cpu.py parses it) ----
enum { QS_PAL_HALF = 16, QS_PAL_OUTSIDE = 32, QS_PAL_INSIDE = 33, QS_PAL_OBSTACLE = 34, QS_PAL_TARGET = 35,
       QS_PAL_BORDER = 36, QS_PAL_N = 37 };
__constant__ const unsigned char QS_RENDER_PALETTE[QS_PAL_N][3] = {
    {230, 25, 75}, {60, 180, 75}, {255, 225, 25}, {0, 130, 200},
    {245, 130, 48}, {145, 30, 180}, {70, 240, 240}, {240, 50, 230},
    {210, 245, 60}, {250, 190, 212}, {0, 128, 128}, {220, 190, 255},
    {170, 110, 40}, {255, 250, 200}, {128, 0, 0}, {170, 255, 195},
    {115, 12, 37}, {30, 90, 37}, {127, 112, 12}, {0, 65, 100},
    {122, 65, 24}, {72, 15, 90}, {35, 120, 120}, {120, 25, 115},
    {105, 122, 30}, {125, 95, 106}, {0, 64, 64}, {110, 95, 127},
    {85, 55, 20}, {127, 125, 100}, {64, 0, 0}, {85, 127, 97},
    {24, 24, 28}, {52, 54, 60}, {150, 150, 158}, {255, 255, 255},
    {200, 200, 205},
};

enum { QS_VIEW_TOPDOWN = 0, QS_VIEW_SIDE = 1, QS_VIEW_FRONT = 2, QS_VIEW_N = 3 };
enum { QS_RD_NONE = 0, QS_RD_DISC = 1, QS_RD_RING = 2, QS_RD_SEG = 3, QS_RD_RECT = 4 };
constexpr int QS_RD_TW = 64, QS_RD_TH = 16, QS_RD_ROWS = 4, QS_RD_WG = 256;   // tile, rows per wave, lanes
constexpr int QS_RD_PER_DRONE = 9;                    // 4 arms, 2 rear rotors, 2 front rotors, body
constexpr int QS_RD_MAX_OBST = 64, QS_RD_NTARGET = 3; // pillar slots (obst_area^2 <= 64); cross arms + capture ring
constexpr float QS_RD_MARGIN = 4.f, QS_RD_SEG_HW = 0.6f, QS_RD_BORDER_HW = 0.5f + 0.0009765625f;
constexpr float QS_RD_MIN_R = 0.75f, QS_RD_GOAL_R = 0.10f, QS_RD_GOAL_MIN_R = 2.5f, QS_RD_CROSS = 3.f;
constexpr float QS_RD_FOLLOW_PAD = 2.f, QS_RD_ROTOR_R = 0.4f, QS_RD_BODY_R = 0.5f;

// One screen-space primitive (pixel units), 32 bytes.  DISC: (a, b) centre, c radius.  RING: centre, c outer, d inner
// radius.  SEG: (a, b) - (c, d), half width QS_RD_SEG_HW.  RECT: a <= x <= c, b <= y <= d.
struct RPrim {
    int type, color;
    float a, b, c, d;
    int pad[2];
};
static_assert(sizeof(RPrim) == 32, "RPrim is 32 bytes");

struct RenderArgs {
    int W, H, view, follow;
    float drone_scale;
    int n;
};

// primitives a config can produce (the LDS list's capacity) and the kernel's dynamic LDS bytes: the primitives, one
// uint16 index list per wave, the drones' (u, v) for the follow window, the 4 waves' colour rows
__host__ __device__ constexpr int render_max_prims(int N, int M, bool flavor_a) {
    return M + (flavor_a ? QS_RD_NTARGET : N) + QS_RD_PER_DRONE * N;
}
__host__ __device__ constexpr int render_list_stride(int P) { return (P + 63) & ~63; }
__host__ __device__ constexpr size_t render_lds_bytes(int P) {
    return sizeof(RPrim) * (size_t)P + 4 * 2 * (size_t)render_list_stride(P) + 2 * 4 * QS_MAX_AGENTS +
           4 * QS_RD_ROWS * QS_RD_TW * 3;
}

__device__ __forceinline__ float rd_wave_sum(float v) {   // xor butterfly: one fixed order, every lane gets the sum
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}
__device__ __forceinline__ float rd_wave_max(float v) {
    for (int m = 32; m >= 1; m >>= 1) v = fmaxf(v, __shfl_xor(v, m, 64));
    return v;
}

__device__ __forceinline__ RPrim rd_prim(int type, int color, float a, float b, float c, float d) {
    RPrim p;
    p.type = type; p.color = color; p.a = a; p.b = b; p.c = c; p.d = d; p.pad[0] = p.pad[1] = 0;
    return p;
}

// does the primitive's bounding box (grown by a hundredth of a pixel: culling may only err towards keeping) meet the
// rectangle [x0, x1] x [y0, y1] of pixel centres?  Non-finite primitives compare false and are dropped.
__device__ __forceinline__ bool rd_bbox_hit(const RPrim& p, float x0, float y0, float x1, float y1) {
    float bx0, by0, bx1, by1;
    if (p.type == QS_RD_DISC || p.type == QS_RD_RING) {
        bx0 = p.a - p.c; bx1 = p.a + p.c; by0 = p.b - p.c; by1 = p.b + p.c;
    } else if (p.type == QS_RD_SEG) {
        bx0 = fminf(p.a, p.c) - QS_RD_SEG_HW; bx1 = fmaxf(p.a, p.c) + QS_RD_SEG_HW;
        by0 = fminf(p.b, p.d) - QS_RD_SEG_HW; by1 = fmaxf(p.b, p.d) + QS_RD_SEG_HW;
    } else if (p.type == QS_RD_RECT) {
        bx0 = p.a; by0 = p.b; bx1 = p.c; by1 = p.d;
    } else {
        return false;
    }
    const float e = 0.01f;
    return bx0 - e <= x1 && bx1 + e >= x0 && by0 - e <= y1 && by1 + e >= y0;
}

__device__ __forceinline__ bool rd_covers(const RPrim& p, float x, float y) {
    if (p.type == QS_RD_RECT) return x >= p.a && x <= p.c && y >= p.b && y <= p.d;
    const float dx = x - p.a, dy = y - p.b;
    if (p.type == QS_RD_SEG) {
        const float ex = p.c - p.a, ey = p.d - p.b, l2 = ex * ex + ey * ey;
        float t = l2 > 0.f ? (dx * ex + dy * ey) / l2 : 0.f;
        t = fminf(fmaxf(t, 0.f), 1.f);
        const float qx = dx - t * ex, qy = dy - t * ey;
        return qx * qx + qy * qy <= QS_RD_SEG_HW * QS_RD_SEG_HW;
    }
    const float d2 = dx * dx + dy * dy;
    if (p.type == QS_RD_DISC) return d2 <= p.c * p.c;
    return d2 <= p.c * p.c && d2 >= p.d * p.d;   // ring
}

// distance from (x, y) to the outline of the rectangle [x0, x1] x [y0, y1], compared with hw
__device__ __forceinline__ bool rd_on_outline(float x, float y, float x0, float y0, float x1, float y1, float hw) {
    const float ox = fmaxf(fmaxf(x0 - x, x - x1), 0.f), oy = fmaxf(fmaxf(y0 - y, y - y1), 0.f);
    if (ox > 0.f || oy > 0.f) return ox * ox + oy * oy <= hw * hw;
    return fminf(fminf(x - x0, x1 - x), fminf(y - y0, y1 - y)) <= hw;
}

__global__ __launch_bounds__(QS_RD_WG) void render_kernel(const KP* __restrict__ kpp, const float* __restrict__ st,
                                                          const int32_t* __restrict__ ist, const int32_t* __restrict__ env,
                                                          const float* __restrict__ envf, const float2* __restrict__ obst,
                                                          const int32_t* __restrict__ env_ids, uint32_t* __restrict__ rgb,
                                                          RenderArgs ra) {
    extern __shared__ __align__(16) unsigned char rd_lds[];
    const KP& kp = *kpp;
    const int N = kp.N, E = kp.E, I = kp.I;
    const bool FA = kp.flavor == QS_FLAVOR_A;
    const int M = kp.obst ? min(kp.M, QS_RD_MAX_OBST) : 0;
    const int P = render_max_prims(N, M, FA), LS = render_list_stride(P);
    RPrim* prim = (RPrim*)rd_lds;
    uint16_t* lists = (uint16_t*)(rd_lds + sizeof(RPrim) * (size_t)P);
    float* su = (float*)(lists + 4 * LS);
    float* sv = su + QS_MAX_AGENTS;
    unsigned char* rows = (unsigned char*)(sv + QS_MAX_AGENTS);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tiles_x = (ra.W + QS_RD_TW - 1) / QS_RD_TW;
    const int tx = blockIdx.x % tiles_x, ty = blockIdx.x / tiles_x;
    const int slot = blockIdx.y;                                   // which selected env: < ra.n by the grid
    const int e = min(max(env_ids[slot], 0), E - 1);               // a bad id can never read out of bounds
    const int iu = ra.view == QS_VIEW_FRONT ? 1 : 0, iv = ra.view == QS_VIEW_TOPDOWN ? 1 : 2;
    const float Wf = (float)ra.W, Hf = (float)ra.H, ds = ra.drone_scale;

    // ---- stage 1: the env's drones, one per lane (field-major state: consecutive lanes, consecutive words) ----
    const bool live = tid < N;
    const int g = e * N + (live ? tid : 0);
    float pu = 0.f, pv = 0.f;
    if (live) {
        pu = st[(QS_F_POS + iu) * I + g];
        pv = st[(QS_F_POS + iv) * I + g];
        su[tid] = pu;
        sv[tid] = pv;
    }
    float cu = 0.5f * (kp.room_lo[iu] + kp.room_hi[iu]), cv = 0.5f * (kp.room_lo[iv] + kp.room_hi[iv]);
    float span_u = kp.room_hi[iu] - kp.room_lo[iu], span_v = kp.room_hi[iv] - kp.room_lo[iv];
    if (ra.follow) {
        // every wave reduces the same values in the same order: no broadcast, and two renders agree bitwise
        __syncthreads();
        const bool h0 = lane < N, h1 = lane + 64 < N;
        const float inv_n = 1.f / (float)N;
        cu = rd_wave_sum((h0 ? su[lane] : 0.f) + (h1 ? su[lane + 64] : 0.f)) * inv_n;
        cv = rd_wave_sum((h0 ? sv[lane] : 0.f) + (h1 ? sv[lane + 64] : 0.f)) * inv_n;
        float r = 0.f;
        if (h0) r = fmaxf(fabsf(su[lane] - cu), fabsf(sv[lane] - cv));
        if (h1) r = fmaxf(r, fmaxf(fabsf(su[lane + 64] - cu), fabsf(sv[lane + 64] - cv)));
        r = rd_wave_max(r);
        span_u = span_v = fmaxf(2.f * r + QS_RD_FOLLOW_PAD, QS_RD_FOLLOW_PAD);
    }
    const float s = fminf((Wf - 2.f * QS_RD_MARGIN) / span_u, (Hf - 2.f * QS_RD_MARGIN) / span_v);
    const float hw_ = 0.5f * Wf, hh_ = 0.5f * Hf;
#define QS_RD_X(u) (hw_ + ((u) - cu) * s)
#define QS_RD_Y(v) (hh_ - ((v) - cv) * s)
    const float rx0 = QS_RD_X(kp.room_lo[iu]), rx1 = QS_RD_X(kp.room_hi[iu]);
    const float ry0 = QS_RD_Y(kp.room_hi[iv]), ry1 = QS_RD_Y(kp.room_lo[iv]);

    // layer order: pillars, target, goal rings, drones
    int n_obst = 0, osi = 0;
    if (M > 0) {
        int omi = 0;
        if (kp.dr) {
            omi = min(max(env[QS_E_OBST_M * E + e], 0), 8);
            osi = min(max(env[QS_E_OBST_SZ * E + e], 0), 8);
        }
        n_obst = min(max(kp.dr_m[omi], 0), M);
    }
    const int n_tgt = FA ? (ra.view == QS_VIEW_TOPDOWN ? 3 : 2) : 0;
    const int goal0 = n_obst + n_tgt, drone0 = goal0 + (FA ? 0 : N), n_prim = drone0 + QS_RD_PER_DRONE * N;

    if (live) {
        const int fl = ist[QS_I_FLAGS * I + g];
        const int full = (tid & 15) + ((fl & QS_FL_ON_FLOOR) ? QS_PAL_HALF : 0), half = (tid & 15) + QS_PAL_HALF;
        const float x = QS_RD_X(pu), y = QS_RD_Y(pv);
        if (!FA) {
            const float gx = QS_RD_X(st[(QS_F_GOAL + iu) * I + g]), gy = QS_RD_Y(st[(QS_F_GOAL + iv) * I + g]);
            const float ro = fmaxf(QS_RD_GOAL_R * ds * s, QS_RD_GOAL_MIN_R);
            prim[goal0 + tid] = rd_prim(QS_RD_RING, full, gx, gy, ro, ro - 1.f);
        }
        // rotor k at pos + drone_scale R (arm / sqrt 2 (sx, sy, 0)): columns 0 and 1 of the row-major rotation
        const float a = kp.arm * 0.70710678f * ds;
        const float ru0 = st[(QS_F_ROT + 3 * iu) * I + g], ru1 = st[(QS_F_ROT + 3 * iu + 1) * I + g];
        const float rv0 = st[(QS_F_ROT + 3 * iv) * I + g], rv1 = st[(QS_F_ROT + 3 * iv + 1) * I + g];
        RPrim* dp = prim + drone0 + QS_RD_PER_DRONE * tid;
        const float rr = fmaxf(QS_RD_ROTOR_R * kp.arm * ds * s, QS_RD_MIN_R);
        const float rb = fmaxf(QS_RD_BODY_R * kp.arm * ds * s, QS_RD_MIN_R);
        for (int k = 0; k < 4; ++k) {   // k: rear (-x) pair first, then the front (+x) pair
            const float sx = k < 2 ? -1.f : 1.f, sy = (k & 1) ? -1.f : 1.f;
            const float qx = x + (a * (sx * ru0 + sy * ru1)) * s, qy = y - (a * (sx * rv0 + sy * rv1)) * s;
            dp[k] = rd_prim(QS_RD_SEG, full, x, y, qx, qy);
            dp[4 + k] = rd_prim(QS_RD_DISC, k < 2 ? half : full, qx, qy, rr, 0.f);
        }
        dp[8] = rd_prim(QS_RD_DISC, full, x, y, rb, 0.f);
    } else if (tid >= 128 && tid < 128 + n_obst) {
        const float2 o = obst[(size_t)e * kp.M + (tid - 128)];
        const float r = kp.dr_r[osi] * s;
        if (ra.view == QS_VIEW_TOPDOWN) {
            prim[tid - 128] = rd_prim(QS_RD_DISC, QS_PAL_OBSTACLE, QS_RD_X(o.x), QS_RD_Y(o.y), r, 0.f);
        } else {
            const float c = QS_RD_X(iu == 0 ? o.x : o.y);
            prim[tid - 128] = rd_prim(QS_RD_RECT, QS_PAL_OBSTACLE, c - r, QS_RD_Y(kp.room_hi[2]), c + r, QS_RD_Y(kp.room_lo[2]));
        }
    } else if (tid == 192 && FA) {
        const float tgx = envf[QS_ENVF_TARGET_X * E + e], tgy = envf[QS_ENVF_TARGET_Y * E + e];
        const float tgz = fmaxf(kp.tgt_z, 0.25f);                  // the height the step kernel gives the target
        const float x = QS_RD_X(iu == 0 ? tgx : tgy), y = QS_RD_Y(iv == 1 ? tgy : tgz);
        prim[n_obst] = rd_prim(QS_RD_SEG, QS_PAL_TARGET, x - QS_RD_CROSS, y, x + QS_RD_CROSS, y);
        prim[n_obst + 1] = rd_prim(QS_RD_SEG, QS_PAL_TARGET, x, y - QS_RD_CROSS, x, y + QS_RD_CROSS);
        if (n_tgt == 3) {
            const float ro = envf[QS_ENVF_CAPTURE * E + e] * s;
            prim[n_obst + 2] = rd_prim(QS_RD_RING, QS_PAL_TARGET, x, y, ro, fmaxf(ro - 1.f, 0.f));
        }
    }
#undef QS_RD_X
#undef QS_RD_Y
    __syncthreads();

    // ---- stage 2: this wave's primitives, in layer order ----
    const int col = tx * QS_RD_TW + lane, row0 = ty * QS_RD_TH + wave * QS_RD_ROWS;
    const float wx0 = (float)(tx * QS_RD_TW) + 0.5f, wx1 = wx0 + (float)(QS_RD_TW - 1);
    const float wy0 = (float)row0 + 0.5f, wy1 = wy0 + (float)(QS_RD_ROWS - 1);
    uint16_t* list = lists + wave * LS;
    int kept = 0;                                                  // wave-uniform
    for (int base = 0; base < n_prim; base += 64) {
        const int i = base + lane;
        const bool hit = i < n_prim && rd_bbox_hit(prim[i], wx0, wy0, wx1, wy1);
        const unsigned long long m = __ballot(hit);
        if (hit) list[kept + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u))] = (uint16_t)i;
        kept += __popcll(m);
    }
    __syncthreads();   // (each list is read by the wave that wrote it; the barrier only orders its LDS writes)

    // ---- stage 3: shade 4 pixels per lane, colours to LDS ----
    const float px = (float)col + 0.5f;
    int colr[QS_RD_ROWS];
    bool in_x = px >= rx0 && px <= rx1;
    for (int r = 0; r < QS_RD_ROWS; ++r) {
        const float py = (float)(row0 + r) + 0.5f;
        colr[r] = (in_x && py >= ry0 && py <= ry1) ? QS_PAL_INSIDE : QS_PAL_OUTSIDE;
    }
    for (int k = 0; k < kept; ++k) {
        const RPrim p = prim[list[k]];                             // the same address on every lane: a broadcast
        for (int r = 0; r < QS_RD_ROWS; ++r)
            if (rd_covers(p, px, (float)(row0 + r) + 0.5f)) colr[r] = p.color;
    }
    unsigned char* wrow = rows + wave * (QS_RD_ROWS * QS_RD_TW * 3);
    for (int r = 0; r < QS_RD_ROWS; ++r) {
        if (rd_on_outline(px, (float)(row0 + r) + 0.5f, rx0, ry0, rx1, ry1, QS_RD_BORDER_HW)) colr[r] = QS_PAL_BORDER;
        const unsigned char* c = QS_RENDER_PALETTE[colr[r]];
        unsigned char* d = wrow + (r * QS_RD_TW + lane) * 3;
        d[0] = c[0]; d[1] = c[1]; d[2] = c[2];
    }
    __syncthreads();

    // ---- store: 48 dwords per row, whole dwords only (W % 4 == 0: every row starts and ends on one) ----
    const int cols_valid = min(QS_RD_TW, ra.W - tx * QS_RD_TW);    // a multiple of 4
    const int dw_valid = cols_valid * 3 / 4;
    constexpr int DW_ROW = QS_RD_TW * 3 / 4;
    const uint32_t* wdw = (const uint32_t*)wrow;
    for (int d = lane; d < QS_RD_ROWS * DW_ROW; d += 64) {
        const int r = d / DW_ROW, w = d - r * DW_ROW, row = row0 + r;
        if (row < ra.H && w < dw_valid)
            rgb[(((size_t)slot * ra.H + row) * ra.W + (size_t)tx * QS_RD_TW) * 3 / 4 + w] = wdw[d];
    }
}

}  // namespace qs
