// Posing a rest-pose scene on the device, and the compact (one constant per triangle and channel) texture form.
//
// rf_pose_scene: per-object affine transforms and a material table turn a rig's rest triangles / normals / ids
// into the triangles, vn and [rows, C] material rows of one frame, in one launch.  rf_texture_rows: the compact
// counterpart of rf_texture_scan (prologue.hip) for such rows.  Both are launch-bound at the scenes' sizes
// (about 120 B per triangle); they are laid out for coalesced row access and nothing else.
#include <math.h>

#include "common.h"

namespace {

constexpr int POSE_ROWS = 256;  // triangle rows per workgroup, one thread each
constexpr int POSE_MAXC = 16;   // material channels (rf_texture_linear's limit)

// a d - b c of fp32 values in fp64: both products are exact (48-bit), so one rounding at 2^-53
RF_DEV double det2(float a, float b, float c, float d) { return (double)a * (double)d - (double)b * (double)c; }

// A workgroup stages its 256 rows of triangles and normals (9 floats each) through LDS: the global loads and
// stores run over consecutive floats (lane = float), the per-row arithmetic reads its row at stride 9 (odd: no
// bank conflict).  The material rows are gathered with lanes assigned to output floats.
__global__ __launch_bounds__(256) void pose_scene_kernel(
    const float* __restrict__ tris, const float* __restrict__ vn, const int32_t* __restrict__ object_id,
    const int32_t* __restrict__ material_id, const float* __restrict__ xf, int ld_xf,
    const float* __restrict__ materials, int64_t rows, int n_per_scene, int n_obj, int n_mat, int channels,
    float* __restrict__ tris_out, float* __restrict__ vn_out, float* __restrict__ tex_out) {
    __shared__ float sp[POSE_ROWS * 9];
    __shared__ float sn[POSE_ROWS * 9];
    __shared__ int smat[POSE_ROWS];  // row of `materials` (b * n_mat + material id), -1: a zero row
    const int64_t r0 = (int64_t)blockIdx.x * POSE_ROWS;
    const int nr = rows - r0 < POSE_ROWS ? (int)(rows - r0) : POSE_ROWS;
    const int t = threadIdx.x;
    for (int i = t; i < nr * 9; i += 256) {
        sp[i] = tris[r0 * 9 + i];
        sn[i] = vn[r0 * 9 + i];
    }
    __syncthreads();
    if (t < nr) {
        const int64_t r = r0 + t;
        const int b = (int)(r / n_per_scene);
        const int o = object_id[r];
        const int m = material_id[r];
        // (ids outside the tables read nothing: such a row is passed through like a padding row)
        const bool posed = o >= 0 && o < n_obj;
        smat[t] = posed && m >= 0 && m < n_mat ? b * n_mat + m : -1;
        if (posed) {
            const float* a = xf + ((int64_t)b * n_obj + o) * ld_xf;
            const float a00 = a[0], a01 = a[1], a02 = a[2], t0 = a[3];
            const float a10 = a[4], a11 = a[5], a12 = a[6], t1 = a[7];
            const float a20 = a[8], a21 = a[9], a22 = a[10], t2 = a[11];
            // cof(A): rows a1 x a2, a2 x a0, a0 x a1; det A = a0 . (a1 x a2)
            double c00 = det2(a11, a12, a21, a22), c01 = det2(a12, a10, a22, a20), c02 = det2(a10, a11, a20, a21);
            double c10 = det2(a21, a22, a01, a02), c11 = det2(a22, a20, a02, a00), c12 = det2(a20, a21, a00, a01);
            double c20 = det2(a01, a02, a11, a12), c21 = det2(a02, a00, a12, a10), c22 = det2(a00, a01, a10, a11);
            const double det = (double)a00 * c00 + (double)a01 * c01 + (double)a02 * c02;
            if (det < 0.0) {
                c00 = -c00, c01 = -c01, c02 = -c02;
                c10 = -c10, c11 = -c11, c12 = -c12;
                c20 = -c20, c21 = -c21, c22 = -c22;
            }
            float* p = sp + t * 9;
            float* n = sn + t * 9;
#pragma unroll
            for (int v = 0; v < 3; ++v) {
                const float x = p[3 * v], y = p[3 * v + 1], z = p[3 * v + 2];
                p[3 * v] = fmaf(a02, z, fmaf(a01, y, fmaf(a00, x, t0)));
                p[3 * v + 1] = fmaf(a12, z, fmaf(a11, y, fmaf(a10, x, t1)));
                p[3 * v + 2] = fmaf(a22, z, fmaf(a21, y, fmaf(a20, x, t2)));
                const double nx = n[3 * v], ny = n[3 * v + 1], nz = n[3 * v + 2];
                const double gx = c00 * nx + c01 * ny + c02 * nz;
                const double gy = c10 * nx + c11 * ny + c12 * nz;
                const double gz = c20 * nx + c21 * ny + c22 * nz;
                const double len = sqrt(gx * gx + gy * gy + gz * gz);
                const bool ok = len > 0.0;  // (false for a NaN too)
                n[3 * v] = ok ? (float)(gx / len) : 0.f;
                n[3 * v + 1] = ok ? (float)(gy / len) : 0.f;
                n[3 * v + 2] = ok ? (float)(gz / len) : 0.f;
            }
        }
    }
    __syncthreads();
    for (int i = t; i < nr * 9; i += 256) {
        tris_out[r0 * 9 + i] = sp[i];
        vn_out[r0 * 9 + i] = sn[i];
    }
    for (int i = t; i < nr * channels; i += 256) {
        const int rr = i / channels, ch = i - rr * channels;
        const int m = smat[rr];
        tex_out[r0 * channels + i] = m >= 0 ? materials[(int64_t)m * channels + ch] : 0.f;
    }
}

// lane = float of the [rows, channels] texture: the last log_channels of every row are log-encoded in place with
// texture_scan_kernel's expression, and a valid row's constants go to its coef row.
__global__ __launch_bounds__(256) void texture_rows_kernel(float* __restrict__ tex, int64_t total, int channels,
                                                           int log_from, const int32_t* __restrict__ dst_row,
                                                           float* __restrict__ coef, int64_t ldc) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int64_t r = i / channels;
    const int ch = (int)(i - r * channels);
    float v = tex[i];
    if (ch >= log_from) {
        v = log10f(v + 1.0f);
        tex[i] = v;
    }
    const int d = dst_row ? dst_row[r] : (int)r;
    if (d >= 0) coef[(int64_t)d * ldc + ch] = v;
}

}  // namespace

extern "C" int rf_pose_scene(const float* tris, const float* vn, const int32_t* object_id, const int32_t* material_id,
                             const float* xf, int ld_xf, const float* materials, int n_scenes, int n_tris_per_scene,
                             int n_objects, int n_materials, int channels, float* tris_out, float* vn_out,
                             float* tex_out, void* stream) {
    RF_REQUIRE(n_scenes >= 0 && n_tris_per_scene >= 0 && n_objects >= 0 && n_materials >= 0 && channels >= 0,
               "rf_pose_scene: negative count (scenes %d, triangles %d, objects %d, materials %d, channels %d)",
               n_scenes, n_tris_per_scene, n_objects, n_materials, channels);
    RF_REQUIRE(ld_xf == 12 || ld_xf == 16, "rf_pose_scene: ld_xf must be 12 or 16 (got %d)", ld_xf);
    RF_REQUIRE(channels <= POSE_MAXC, "rf_pose_scene: at most %d material channels (got %d)", POSE_MAXC, channels);
    const int64_t rows = (int64_t)n_scenes * n_tris_per_scene;
    RF_REQUIRE(rows < (1ll << 31) && (int64_t)n_scenes * n_materials < (1ll << 31),
               "rf_pose_scene: n_scenes * n_tris_per_scene and n_scenes * n_materials must stay below 2^31");
    if (rows == 0) return RF_OK;
    RF_REQUIRE(tris && vn && object_id && material_id && tris_out && vn_out,
               "rf_pose_scene: null pointer (tris, vn, object_id, material_id, tris_out, vn_out)");
    RF_REQUIRE(xf || n_objects == 0, "rf_pose_scene: null xf with %d objects", n_objects);
    RF_REQUIRE(channels == 0 || tex_out, "rf_pose_scene: null tex_out with %d channels", channels);
    RF_REQUIRE(materials || n_materials == 0 || channels == 0, "rf_pose_scene: null materials");
    RF_LAUNCH(pose_scene_kernel, dim3((unsigned)((rows + POSE_ROWS - 1) / POSE_ROWS)), dim3(256), 0,
              (hipStream_t)stream, tris, vn, object_id, material_id, xf, ld_xf, materials, rows, n_tris_per_scene,
              n_objects, n_materials, channels, tris_out, vn_out, tex_out);
    return rf::check_launch("rf_pose_scene");
}

extern "C" int rf_texture_rows(float* texture, int64_t n_rows, int channels, int log_channels,
                               const int32_t* dst_row, float* coef, int64_t ldc, void* stream) {
    RF_REQUIRE(n_rows >= 0 && n_rows < (1ll << 31), "rf_texture_rows: need 0 .. 2^31 rows");
    RF_REQUIRE(channels >= 1 && channels <= POSE_MAXC && ldc >= channels,
               "rf_texture_rows: channels must be in [1, %d] and ldc >= channels", POSE_MAXC);
    RF_REQUIRE(log_channels >= 0 && log_channels <= channels, "rf_texture_rows: bad log_channels");
    if (n_rows == 0) return RF_OK;
    RF_REQUIRE(texture && coef, "rf_texture_rows: null pointer");
    const int64_t total = n_rows * channels;
    RF_LAUNCH(texture_rows_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, texture,
              total, channels, channels - log_channels, dst_row, coef, ldc);
    return rf::check_launch("rf_texture_rows");
}
