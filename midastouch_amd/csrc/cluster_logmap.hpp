// cluster_logmap.hpp - the log-map form of a cluster centre (particle_filter.get_cluster_centers(method="logmap"),
// modules/particle_filter.py:153-206 with pose.log_map_averaged, modules/pose.py:101-109): the weighted mean of the members'
// se(3) logarithms, mapped back with the exponential.  DESIGN.md 2, "The log-map centre's arithmetic".  Shared by the per-particle
// kernel (k_se3_log), the moment accumulation and the finishers of cluster.hip.
#pragma once
#include "midas_internal.hpp"
#include "midas_math.hpp"
#include "cluster_rot.hpp"

namespace midas {

// The log-map form keeps the 36-slot record (CL_MOM: scratch sizes and the partials' layout are the quaternion form's): the six
// sums of w xi lie where the ten of w q q^T begin, the six of xi where those of q q^T begin; the four slots behind each stay +0.0.
enum : int {
    M_XW = M_QQW,  // 6: sum w xi, xi = [u, omega]
    M_X1 = M_QQ1,  // 6: sum xi
};
constexpr int CL_FORM_QUAT = 0, CL_FORM_LOGMAP = 1;

// xi = [V^-1 t, omega] of a row-major pose, float64 from the float32 entries: omega is so3_log's float32 vector widened, the rest
// pose.se3_log's formulas and threshold in its order of operations
MD void se3_log_f64(const float* P, double* xi) {
    float wf[3];
    so3_log(P, wf);
    const double ox = (double)wf[0], oy = (double)wf[1], oz = (double)wf[2];
    const double tx = (double)P[3], ty = (double)P[7], tz = (double)P[11];
    const double th = __builtin_sqrt((ox * ox + oy * oy) + oz * oz);
    const double h = 0.5 * th;
    const double c = th > 1e-6 ? (1.0 - h * cos(h) / sin(h)) / (th * th) : 1.0 / 12.0;
    const double ax = oy * tz - oz * ty, ay = oz * tx - ox * tz, az = ox * ty - oy * tx;  // a = omega x t
    const double bx = oy * az - oz * ay, by = oz * ax - ox * az, bz = ox * ay - oy * ax;  // omega x a
    xi[0] = (tx - 0.5 * ax) + c * bx;
    xi[1] = (ty - 0.5 * ay) + c * by;
    xi[2] = (tz - 0.5 * az) + c * bz;
    xi[3] = ox; xi[4] = oy; xi[5] = oz;
}

// cluster_close's twin: one cluster from its summed moments (one thread).  Count, empty label, float32 weights' flatten rule and
// the NaN rule are cluster_close's; the centre is exp(sum w xi / sum w) - rotation AND translation, all sixteen entries are written
// here - and the spread the same closed form around the float32 centre translation, which is not the weighted mean translation.
MD void cluster_close_logmap(const double* s_m, float* out, float* sd, int64_t* count) {
    if (count) *count = (int64_t)s_m[M_CNT];
    if (s_m[M_CNT] == 0.0) {
        for (int i = 0; i < 16; ++i) out[i] = NAN;
        for (int i = 0; i < 3; ++i) sd[i] = NAN;
        return;
    }
    const float d = (float)s_m[M_WMAX] - (float)s_m[M_WMIN];
    const bool flat = __builtin_fabsf(d) <= 1e-8f && s_m[M_SW] == s_m[M_SW];
    const int ox = flat ? M_X1 : M_XW, ot = flat ? M_T1 : M_TW, ott = flat ? M_TT1 : M_TTW;
    const double sw = flat ? s_m[M_CNT] : s_m[M_SW];
    double xb[6];
    for (int k = 0; k < 6; ++k) xb[k] = s_m[ox + k] / sw;
    const double wx = xb[3], wy = xb[4], wz = xb[5];
    const double th = __builtin_sqrt((wx * wx + wy * wy) + wz * wz);
    double A = 1.0, B = 0.5, Cc = 1.0 / 6.0;
    if (!(th <= 1e-8)) {  // (NaN: the closed forms, NaN out)
        const double s = sin(th), c = cos(th);
        A = s / th; B = (1.0 - c) / (th * th); Cc = (th - s) / (th * th * th);
    }
    const double W[9] = {0.0, -wz, wy, wz, 0.0, -wx, -wy, wx, 0.0};
    double W2[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) W2[i * 3 + j] = (W[i * 3] * W[j] + W[i * 3 + 1] * W[3 + j]) + W[i * 3 + 2] * W[6 + j];
    float mean[3];
    for (int i = 0; i < 3; ++i) {
        double tv = 0.0;
        for (int j = 0; j < 3; ++j) {
            const double e = i == j ? 1.0 : 0.0;
            out[i * 4 + j] = (float)((e + A * W[i * 3 + j]) + B * W2[i * 3 + j]);
            tv = tv + ((e + B * W[i * 3 + j]) + Cc * W2[i * 3 + j]) * xb[j];
        }
        mean[i] = (float)tv;
        out[i * 4 + 3] = mean[i];
    }
    out[12] = 0.f; out[13] = 0.f; out[14] = 0.f; out[15] = 1.f;
    for (int i = 0; i < 3; ++i) {
        const double m = (double)mean[i];
        double var = (s_m[ott + i] - 2.0 * m * s_m[ot + i] + m * m * sw) / sw;
        var = var < 0.0 ? 0.0 : var;
        sd[i] = (float)__builtin_sqrt(var);
    }
}

}  // namespace midas
