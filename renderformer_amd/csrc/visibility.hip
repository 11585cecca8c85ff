// Geometry buffers from primary rays (rf.h rf_primary_hits / rf_gbuffer_shade): brute-force nearest-hit visibility of
// the pixel rays of ray_tokens_cam_kernel (prologue.hip) against a scene's valid triangles, and the elementwise
// shading of (tri_id, bary) into alpha / normal / albedo.  Both only read their inputs.
//
// Arithmetic.  With o the view's origin and a, b, c = v0 - o, v1 - o, v2 - o (fp32, so a vertex shared bit for bit
// stays shared), the edge functions of a ray direction d are
//   E0 = d . (b x c)   E1 = d . (c x a)   E2 = d . (a x b)
// and the ray passes inside the triangle iff all three are >= 0 or all are <= 0 (double-sided, closed edges).  They
// decide coverage only: their error is 2^-24 |p| |q| against a sum E0 + E1 + E2 of the size of the triangle's solid
// angle, too coarse for the barycentrics of a small, distant triangle.  A pair that passes is finished with
// Moeller-Trumbore on the edge vectors e1 = v1 - v0, e2 = v2 - v0 of the input coordinates (exact differences up to
// one rounding): det = e1 . (d x e2), u = -a . (d x e2) / det, q = e1 x a, v = d . q / det, t = e2 . q / det, and the
// triangle is hit iff det != 0 and t > 0.
// Watertightness:
//   - an edge's normal p x q is computed with its two vertices in a canonical (lexicographic) order and negated
//     exactly if that swapped them, so the two triangles of a shared edge evaluate the same number with opposite
//     signs, whatever their winding: a ray between them is never rejected by both;
//   - an edge function with |E| <= VIS_EDGE_EPS |p| |q| is evaluated again in fp64 from the same fp32 p, q, d (products
//     of two fp32 values are exact in fp64).  The fp32 value's error is at most ~5 2^-24 |p| |q| (two rounded products
//     per normal component, three FMAs), an eighth of the threshold, so above it the fp32 sign is the fp64 sign; the
//     threshold depends on the edge alone, so both triangles of an edge take the same path.  This makes the signs
//     round a vertex fan mutually consistent (a ray through a vertex is within the threshold of every edge of the fan).
// The trace kernel walks a view's records in index order with a strict < on t: among equal t the lowest index wins,
// and a thread owns its pixel from the first record to the last, so there is no cross-chunk reduction to order.
#include "common.h"
#include "env.h"

namespace {

constexpr int VIS_CHUNK = RF_VIS_CHUNK;  // records staged in LDS per round (one per thread)
constexpr int VIS_TILE = RF_VIS_TILE;    // a workgroup's pixel tile is VIS_TILE x VIS_TILE
constexpr float VIS_EDGE_EPS = 2.5e-6f;
constexpr int VIS_STAGE_DEFAULT = 1;  // RF_VIS_STAGE: 1 stages the records in LDS, 0 reads them through scalar loads
static_assert(VIS_CHUNK == 256 && VIS_TILE * VIS_TILE == 256, "one record and one pixel per thread of a 256-thread block");

// One record per (scene, view, valid triangle): 12 floats the trace loop reads for every pixel ...
struct alignas(16) VisRec {
    float n0[3], n1[3], n2[3];  // b x c, c x a, a x b
    float thr;                  // max of the three edge thresholds; < 0: a dead record (never hit, no fp64 path)
    int id;                     // index on the input N axis of triangles[b]
    int pad;
};
// ... and 20 more that only the fp64 path and a pair that passes the inside test read
struct alignas(16) VisAux {
    float a[3], b[3], c[3];
    float thr[3];  // VIS_EDGE_EPS |b| |c|, |c| |a|, |a| |b|
    float e1[3], e2[3];
    float pad[2];
};
static_assert(sizeof(VisRec) == 48 && sizeof(VisAux) == 80, "rf.h documents 32 floats per record");

RF_DEV bool lex_less(const float* p, const float* q) {
    if (p[0] != q[0]) return p[0] < q[0];
    if (p[1] != q[1]) return p[1] < q[1];
    return p[2] < q[2];
}

// p x q with the vertices in canonical order, negated exactly afterwards if that swapped them
RF_DEV void edge_normal(const float* p, const float* q, float* n) {
    const bool sw = lex_less(q, p);
    const float* lo = sw ? q : p;
    const float* hi = sw ? p : q;
    const float x = lo[1] * hi[2] - lo[2] * hi[1];
    const float y = lo[2] * hi[0] - lo[0] * hi[2];
    const float z = lo[0] * hi[1] - lo[1] * hi[0];
    n[0] = sw ? -x : x;
    n[1] = sw ? -y : y;
    n[2] = sw ? -z : z;
}

// d . (p x q) in fp64 from the fp32 values, in the same canonical order
RF_DEV double edge_fn64(const float* p, const float* q, float dx, float dy, float dz) {
    const bool sw = lex_less(q, p);
    const float* lo = sw ? q : p;
    const float* hi = sw ? p : q;
    // (each product of two fp32 values is exact, so a component is the exact difference rounded once; the dot
    // product is written as explicit FMAs so that every edge slot of every triangle evaluates it in one order)
    const double x = (double)lo[1] * (double)hi[2] - (double)lo[2] * (double)hi[1];
    const double y = (double)lo[2] * (double)hi[0] - (double)lo[0] * (double)hi[2];
    const double z = (double)lo[0] * (double)hi[1] - (double)lo[1] * (double)hi[0];
    const double e = __builtin_fma((double)dx, x, __builtin_fma((double)dy, y, (double)dz * z));
    return sw ? -e : e;
}

RF_DEV float len3(const float* p) { return sqrtf(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]); }

// scene of the global valid index g: the last b with scene_off[b] <= g (empty scenes repeat an offset)
RF_DEV int scene_of(const int32_t* __restrict__ scene_off, int n_scenes, int g) {
    int lo = 0, hi = n_scenes - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (scene_off[mid] <= g) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// rec / aux [sum_b n_views n_b]: scene b's block starts at scene_off[b] n_views, view v's rows at + v n_b.
__global__ __launch_bounds__(256) void vis_setup_kernel(const float* __restrict__ tris,
                                                        const int32_t* __restrict__ valid_idx,
                                                        const int32_t* __restrict__ scene_off,
                                                        const float* __restrict__ c2w, int n_scenes, int n_views,
                                                        int n_per_scene, int n_valid, VisRec* __restrict__ rec,
                                                        VisAux* __restrict__ aux) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    const int view = blockIdx.y;
    if (g >= n_valid) return;
    const int b = scene_of(scene_off, n_scenes, g);
    const int off = scene_off[b];
    const int n_b = min(scene_off[b + 1], n_valid) - off;
    if (off < 0 || g - off >= n_b) return;  // (a scene_off that is not ascending: nothing is written past the tables)
    const int64_t slot = (int64_t)off * n_views + (int64_t)view * n_b + (g - off);
    const int row = valid_idx[g];
    const int id = row - b * n_per_scene;
    VisRec r;
    VisAux x;
    bool live = id >= 0 && id < n_per_scene;  // (a row of another scene is never read)
    const float* m = c2w + ((int64_t)b * n_views + view) * 16;
    const float o[3] = {m[3], m[7], m[11]};
    if (live) {
        const float* t = tris + (int64_t)row * 9;
        double e1[3], e2[3];
        for (int k = 0; k < 3; ++k) {
            x.a[k] = t[k] - o[k];
            x.b[k] = t[3 + k] - o[k];
            x.c[k] = t[6 + k] - o[k];
            live = live && isfinite(x.a[k]) && isfinite(x.b[k]) && isfinite(x.c[k]);
            x.e1[k] = t[3 + k] - t[k];
            x.e2[k] = t[6 + k] - t[k];
            e1[k] = (double)t[3 + k] - (double)t[k];
            e2[k] = (double)t[6 + k] - (double)t[k];
        }
        // zero area: the fp64 cross product of the exact edge vectors vanishes
        const double nx = e1[1] * e2[2] - e1[2] * e2[1], ny = e1[2] * e2[0] - e1[0] * e2[2],
                     nz = e1[0] * e2[1] - e1[1] * e2[0];
        live = live && (nx != 0.0 || ny != 0.0 || nz != 0.0);
    }
    if (live) {
        edge_normal(x.b, x.c, r.n0);
        edge_normal(x.c, x.a, r.n1);
        edge_normal(x.a, x.b, r.n2);
        const float la = len3(x.a), lb = len3(x.b), lc = len3(x.c);
        x.thr[0] = VIS_EDGE_EPS * (lb * lc);
        x.thr[1] = VIS_EDGE_EPS * (lc * la);
        x.thr[2] = VIS_EDGE_EPS * (la * lb);
        r.thr = fmaxf(x.thr[0], fmaxf(x.thr[1], x.thr[2]));
        live = isfinite(r.thr);  // (lengths, and below normals, that overflow fp32)
        for (int k = 0; k < 3; ++k) live = live && isfinite(r.n0[k]) && isfinite(r.n1[k]) && isfinite(r.n2[k]);
    }
    if (!live) {
        for (int k = 0; k < 3; ++k) {
            r.n0[k] = r.n1[k] = r.n2[k] = 0.f;
            x.a[k] = x.b[k] = x.c[k] = x.thr[k] = x.e1[k] = x.e2[k] = 0.f;
        }
        r.thr = -1.f;
    }
    x.pad[0] = x.pad[1] = 0.f;
    r.id = id;
    r.pad = 0;
    rec[slot] = r;
    aux[slot] = x;
}

struct VisHit {
    float t, u, v;
    int id;
};

// one record against one ray; `r` is wave-uniform (LDS broadcast or scalar registers)
RF_DEV void vis_pair(const VisRec& r, const VisAux* __restrict__ aux, float dx, float dy, float dz, VisHit& best) {
    const float e0 = dx * r.n0[0] + dy * r.n0[1] + dz * r.n0[2];
    const float e1 = dx * r.n1[0] + dy * r.n1[1] + dz * r.n1[2];
    const float e2 = dx * r.n2[0] + dy * r.n2[1] + dz * r.n2[2];
    const float lo = fminf(e0, fminf(e1, e2)), hi = fmaxf(e0, fmaxf(e1, e2));
    // Two edge functions of opposite sign, both beyond the largest of the triangle's thresholds: the ray passes outside
    // whatever the third one is, in fp32 and in fp64 alike.  This is how nearly every pair ends (a dead record too:
    // 0 > -1); the rest of the function is the rare path.
    if (fminf(hi, -lo) > r.thr) return;
    const float near = fminf(fabsf(e0), fminf(fabsf(e1), fabsf(e2)));
    bool in = lo >= 0.f || hi <= 0.f;
    if (near <= r.thr) {  // some edge function may be within its threshold: those are evaluated again in fp64
        const double d0 = fabsf(e0) <= aux->thr[0] ? edge_fn64(aux->b, aux->c, dx, dy, dz) : (double)e0;
        const double d1 = fabsf(e1) <= aux->thr[1] ? edge_fn64(aux->c, aux->a, dx, dy, dz) : (double)e1;
        const double d2 = fabsf(e2) <= aux->thr[2] ? edge_fn64(aux->a, aux->b, dx, dy, dz) : (double)e2;
        in = (d0 >= 0.0 && d1 >= 0.0 && d2 >= 0.0) || (d0 <= 0.0 && d1 <= 0.0 && d2 <= 0.0);
    }
    if (in && r.thr >= 0.f) {
        const float* a = aux->a;
        const float* f1 = aux->e1;
        const float* f2 = aux->e2;
        const float p0 = dy * f2[2] - dz * f2[1], p1 = dz * f2[0] - dx * f2[2], p2 = dx * f2[1] - dy * f2[0];
        const float det = f1[0] * p0 + f1[1] * p1 + f1[2] * p2;
        const float q0 = f1[1] * a[2] - f1[2] * a[1], q1 = f1[2] * a[0] - f1[0] * a[2], q2 = f1[0] * a[1] - f1[1] * a[0];
        const float t = (f2[0] * q0 + f2[1] * q1 + f2[2] * q2) / det;
        if (det != 0.f && t > 0.f && t < best.t) {
            best.t = t;
            best.u = -(a[0] * p0 + a[1] * p1 + a[2] * p2) / det;
            best.v = (dx * q0 + dy * q1 + dz * q2) / det;
            best.id = r.id;
        }
    }
}

// A workgroup traces a VIS_TILE x VIS_TILE pixel tile of one view of one scene, a thread one pixel.
// LDS_STAGE: the records are staged VIS_CHUNK at a time in LDS (same-address reads broadcast); otherwise the loop
// reads them from global memory at a wave-uniform address, which the compiler turns into scalar loads.
template <bool LDS_STAGE>
__global__ __launch_bounds__(256) void vis_trace_kernel(const VisRec* __restrict__ rec, const VisAux* __restrict__ aux,
                                                        const int32_t* __restrict__ scene_off,
                                                        const float* __restrict__ c2w, const float* __restrict__ fov,
                                                        const float* __restrict__ intr, int n_views, int n_valid,
                                                        int frame_h, int frame_w, float* __restrict__ depth,
                                                        int32_t* __restrict__ tri_id, float* __restrict__ bary,
                                                        uint8_t* __restrict__ alpha) {
    __shared__ VisRec stage[LDS_STAGE ? VIS_CHUNK : 1];
    const int view = blockIdx.y, b = blockIdx.z;
    const int tiles_x = (frame_w + VIS_TILE - 1) / VIS_TILE;
    const int x = (blockIdx.x % tiles_x) * VIS_TILE + threadIdx.x % VIS_TILE;
    const int y = (blockIdx.x / tiles_x) * VIS_TILE + threadIdx.x / VIS_TILE;
    const bool inside = x < frame_w && y < frame_h;
    const int cam = b * n_views + view;
    // the ray of ray_tokens_cam_kernel (prologue.hip), expression for expression, with x0 = y0 = 0
    const float* m = c2w + (int64_t)cam * 16;
    float fx, fy, cx, cy;
    if (intr) {
        fx = intr[cam * 4 + 0];
        fy = intr[cam * 4 + 1];
        cx = intr[cam * 4 + 2];
        cy = intr[cam * 4 + 3];
    } else {
        const float fov_rad = fov[cam] / 180.0f * 3.14159265358979323846f;
        fx = fy = (float)frame_h / 2.0f / tanf(0.5f * fov_rad);
        cx = (float)frame_w / 2.0f;
        cy = (float)frame_h / 2.0f;
    }
    const float dx = ((float)x + 0.5f - cx) / fx;
    const float dy = -(((float)y + 0.5f - cy) / fy);
    const float dz = -1.0f;
    float r0 = dx * m[0] + dy * m[1] + dz * m[2];
    float r1 = dx * m[4] + dy * m[5] + dz * m[6];
    float r2 = dx * m[8] + dy * m[9] + dz * m[10];
    const float nrm = fmaxf(sqrtf(r0 * r0 + r1 * r1 + r2 * r2), 1e-12f);
    r0 /= nrm;
    r1 /= nrm;
    r2 /= nrm;

    const int off = scene_off[b];
    const int n_b = off < 0 ? 0 : max(min(scene_off[b + 1], n_valid) - off, 0);
    const int64_t base = (int64_t)off * n_views + (int64_t)view * n_b;
    rec += base;
    aux += base;
    VisHit best = {__builtin_inff(), 0.f, 0.f, -1};
    if (LDS_STAGE) {
        for (int k0 = 0; k0 < n_b; k0 += VIS_CHUNK) {
            const int n = min(VIS_CHUNK, n_b - k0);
            __syncthreads();  // the previous round's reads are done
            if ((int)threadIdx.x < n) stage[threadIdx.x] = rec[k0 + threadIdx.x];
            __syncthreads();
#pragma unroll 4
            for (int k = 0; k < n; ++k) vis_pair(stage[k], aux + k0 + k, r0, r1, r2, best);
        }
    } else {
        for (int k = 0; k < n_b; ++k) vis_pair(rec[k], aux + k, r0, r1, r2, best);
    }
    if (!inside) return;
    const int64_t pix = ((int64_t)cam * frame_h + y) * frame_w + x;
    depth[pix] = best.t;
    tri_id[pix] = best.id;
    if (bary) {
        bary[pix * 2] = best.u;
        bary[pix * 2 + 1] = best.v;
    }
    if (alpha) alpha[pix] = best.id >= 0 ? 255 : 0;
}

// (tri_id, bary) -> alpha / normal / albedo, one pixel per thread; pix_per_scene pixels belong to each scene
__global__ __launch_bounds__(256) void gbuffer_shade_kernel(const int32_t* __restrict__ tri_id,
                                                            const float* __restrict__ bary,
                                                            const float* __restrict__ vn,
                                                            const float* __restrict__ texture, int64_t tex_row_stride,
                                                            int64_t tex_chan_stride, int n_per_scene,
                                                            int64_t pix_per_scene, int64_t n_pix,
                                                            uint8_t* __restrict__ alpha, float* __restrict__ normal,
                                                            float* __restrict__ albedo) {
    const int64_t pix = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (pix >= n_pix) return;
    const int id = tri_id[pix];
    const bool hit = id >= 0 && id < n_per_scene;  // (an id outside the scene reads nothing)
    const int64_t row = (pix / pix_per_scene) * n_per_scene + id;
    if (alpha) alpha[pix] = hit ? 255 : 0;
    if (normal) {
        float n0 = 0.f, n1 = 0.f, n2 = 0.f;
        if (hit) {
            const float u = bary[pix * 2], v = bary[pix * 2 + 1], w = 1.0f - u - v;
            const float* q = vn + row * 9;
            n0 = w * q[0] + u * q[3] + v * q[6];
            n1 = w * q[1] + u * q[4] + v * q[7];
            n2 = w * q[2] + u * q[5] + v * q[8];
            const float nrm = fmaxf(sqrtf(n0 * n0 + n1 * n1 + n2 * n2), 1e-12f);
            n0 /= nrm;
            n1 /= nrm;
            n2 /= nrm;
        }
        normal[pix * 3] = n0;
        normal[pix * 3 + 1] = n1;
        normal[pix * 3 + 2] = n2;
    }
    if (albedo) {
        const float* t = texture + row * tex_row_stride;
        albedo[pix * 3] = hit ? t[0] : 0.f;
        albedo[pix * 3 + 1] = hit ? t[tex_chan_stride] : 0.f;
        albedo[pix * 3 + 2] = hit ? t[2 * tex_chan_stride] : 0.f;
    }
}

}  // namespace

extern "C" int rf_primary_hits(const float* tris, const int32_t* valid_idx, const int32_t* scene_off, const float* c2w,
                               const float* fov_deg, const float* intr, int n_scenes, int n_views,
                               int n_tris_per_scene, int64_t n_valid, int frame_h, int frame_w, float* depth,
                               int32_t* tri_id, float* bary, uint8_t* alpha, float* work, int64_t work_floats,
                               void* stream) {
    RF_REQUIRE(tris && valid_idx && scene_off && c2w && depth && tri_id,
               "rf_primary_hits: null pointer (tris, valid_idx, scene_off, c2w, depth, tri_id)");
    RF_REQUIRE((fov_deg != nullptr) != (intr != nullptr), "rf_primary_hits: exactly one of fov_deg and intr");
    RF_REQUIRE(frame_h > 0 && frame_w > 0, "rf_primary_hits: need a positive frame (got %d x %d)", frame_h, frame_w);
    RF_REQUIRE((int64_t)frame_h * frame_w < (1ll << 31), "rf_primary_hits: %d x %d pixels do not fit a 32-bit index",
               frame_h, frame_w);
    RF_REQUIRE(n_views <= 65535, "rf_primary_hits: at most 65535 views per call");
    RF_REQUIRE(n_scenes <= 65535, "rf_primary_hits: at most 65535 scenes per call");
    RF_REQUIRE(n_tris_per_scene > 0 && (int64_t)n_scenes * n_tris_per_scene < (1ll << 31),
               "rf_primary_hits: need 0 < n_tris_per_scene and n_scenes * n_tris_per_scene < 2^31 (got %d x %d)",
               n_scenes, n_tris_per_scene);
    RF_REQUIRE(n_valid >= 0 && n_valid <= (int64_t)(n_scenes > 0 ? n_scenes : 0) * n_tris_per_scene,
               "rf_primary_hits: n_valid %lld outside 0 .. n_scenes * n_tris_per_scene", (long long)n_valid);
    const int64_t need = 32 * (int64_t)(n_views > 0 ? n_views : 0) * n_valid;
    RF_REQUIRE(work_floats >= need && (need == 0 || work),
               "rf_primary_hits: the workspace holds %lld floats, 32 * n_views * n_valid = %lld are needed",
               (long long)work_floats, (long long)need);
    RF_REQUIRE(((uintptr_t)work & 15) == 0, "rf_primary_hits: work must be 16-B aligned");
    if (n_scenes <= 0 || n_views <= 0) return RF_OK;
    VisRec* rec = reinterpret_cast<VisRec*>(work);
    VisAux* aux = reinterpret_cast<VisAux*>(work + 12 * (int64_t)n_views * n_valid);
    hipStream_t st = (hipStream_t)stream;
    if (n_valid > 0) {
        dim3 grid((unsigned)((n_valid + 255) / 256), n_views);
        RF_LAUNCH(vis_setup_kernel, grid, dim3(256), 0, st, tris, valid_idx, scene_off, c2w, n_scenes, n_views,
                  n_tris_per_scene, (int)n_valid, rec, aux);
    }
    const int tiles = ((frame_w + VIS_TILE - 1) / VIS_TILE) * ((frame_h + VIS_TILE - 1) / VIS_TILE);
    dim3 grid(tiles, n_views, n_scenes);
    if (rf::env_int("RF_VIS_STAGE", VIS_STAGE_DEFAULT))
        RF_LAUNCH(vis_trace_kernel<true>, grid, dim3(256), 0, st, rec, aux, scene_off, c2w, fov_deg, intr, n_views,
                  (int)n_valid, frame_h, frame_w, depth, tri_id, bary, alpha);
    else
        RF_LAUNCH(vis_trace_kernel<false>, grid, dim3(256), 0, st, rec, aux, scene_off, c2w, fov_deg, intr, n_views,
                  (int)n_valid, frame_h, frame_w, depth, tri_id, bary, alpha);
    return rf::check_launch("rf_primary_hits");
}

extern "C" int rf_gbuffer_shade(const int32_t* tri_id, const float* bary, const float* vn, const float* texture,
                                int64_t tex_row_stride, int64_t tex_chan_stride, int n_tris_per_scene, int n_scenes,
                                int64_t pix_per_scene, uint8_t* alpha, float* normal, float* albedo, void* stream) {
    RF_REQUIRE(tri_id && (alpha || normal || albedo),
               "rf_gbuffer_shade: null pointer (tri_id, and at least one of alpha, normal and albedo)");
    RF_REQUIRE(!normal || (bary && vn), "rf_gbuffer_shade: normal needs bary and vn");
    RF_REQUIRE(!albedo || texture, "rf_gbuffer_shade: albedo needs texture");
    RF_REQUIRE(!albedo || (tex_chan_stride >= 1 && tex_row_stride >= 2 * tex_chan_stride + 1),
               "rf_gbuffer_shade: a texture row of %lld floats does not hold three channels %lld floats apart",
               (long long)tex_row_stride, (long long)tex_chan_stride);
    RF_REQUIRE(n_tris_per_scene > 0 && (int64_t)(n_scenes > 0 ? n_scenes : 0) * n_tris_per_scene < (1ll << 31),
               "rf_gbuffer_shade: need 0 < n_tris_per_scene and n_scenes * n_tris_per_scene < 2^31 (got %d x %d)",
               n_scenes, n_tris_per_scene);
    RF_REQUIRE(pix_per_scene > 0 && pix_per_scene < (1ll << 40), "rf_gbuffer_shade: need 0 < pix_per_scene < 2^40");
    if (n_scenes <= 0) return RF_OK;
    const int64_t n_pix = pix_per_scene * n_scenes;
    RF_REQUIRE((n_pix + 255) / 256 < (1ll << 31), "rf_gbuffer_shade: too many pixels for one launch");
    RF_LAUNCH(gbuffer_shade_kernel, dim3((unsigned)((n_pix + 255) / 256)), dim3(256), 0, (hipStream_t)stream, tri_id,
              bary, vn, texture, tex_row_stride, tex_chan_stride, n_tris_per_scene, pix_per_scene, n_pix, alpha, normal,
              albedo);
    return rf::check_launch("rf_gbuffer_shade");
}
