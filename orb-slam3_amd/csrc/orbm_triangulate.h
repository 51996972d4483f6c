// orbm_triangulate.h -- the arithmetic of LocalMapping::CreateNewMapPoints for ONE match (LocalMapping.cc:611-892), pinhole cameras,
// NLeft == -1, !mpCamera2, shared by the device (k_triangulate_new, orbm_kernels.hip.h) and by the host tests, which compile this file
// with g++ (tests/triangulate_header.cpp).  Plain IEEE float / double +, -, *, /, sqrt and explicit fma only, built with
// -ffp-contract=off on both sides: the device equals the g++ build bit for bit, x3D included.  No libm call: atan2 and cos are
// restated below so that both builds run the same operations.
//
// Against the REFERENCE the result is held to a tolerance, not to bits: cv::SVD::compute (:768) is replaced by a one-sided
// (Hestenes) Jacobi on the float32 4x4, carried in double and rounded to float32 once (tri_null_vector).  Everything else restates the reference's float
// expressions: cv::Matx products and Matx::dot accumulate in float from 0, cv::norm is the square root of a double sum
// (facade/cvcompat.h states the rules), comparisons against double literals widen the float side.
#pragma once
#include <stdint.h>
#ifndef TRI_FN
#define TRI_FN static inline
#endif

// Every exit of the per-match text.  Values <= TRI_OK_STEREO2 are successes and say which branch of :746-796 made x3D.
enum TriReason {
    TRI_OK_TRIANGULATED = 0,   // :746-781 linear triangulation
    TRI_OK_STEREO1 = 1,        // :782-787 UnprojectStereo_ of KeyFrame 1
    TRI_OK_STEREO2 = 2,        // :788-792 UnprojectStereo_ of KeyFrame 2
    TRI_NO_MATCH = 3,          // matches12 holds no usable idx2 (or the row is out of range)
    TRI_TAKEN = 4,             // the cross-pair rule: an earlier pair turned this idx1 into a MapPoint
    TRI_BAD_OCTAVE = 5,        // an octave outside [0, nlevels): the reference would read past its tables
    TRI_LOW_PARALLAX = 6,      // :793-796 no stereo and very low parallax
    TRI_W_ZERO = 7,            // :772 x3D_h(3) == 0
    TRI_BEHIND_1 = 8,          // :804 z1 <= 0
    TRI_BEHIND_2 = 9,          // :808 z2 <= 0
    TRI_CHI2_1 = 10,           // :825 / :840
    TRI_CHI2_2 = 11,           // :855 / :866
    TRI_DIST_ZERO = 12,        // :880
    TRI_FAR = 13,              // :883
    TRI_SCALE = 14,            // :891
    TRI_MIXED_ROW1 = 15        // the group's pairs do not share one row1 (device form: the group creates nothing)
};
TRI_FN bool tri_ok(int r) { return r <= TRI_OK_STEREO2; }

#define TRI_MAX_LEVELS 32
#define TRI_MAX_SWEEPS 12

struct TriCam { float fx, fy, cx, cy, invfx, invfy; };
struct TriPose { float T[12]; float ow[3]; };                    // row-major 3x4 [Rcw | tcw] and the camera centre
struct TriObs { float ux, uy; float kx, ky; int octave; float uright, depth; };   // mvKeysUn pt, mvKeys pt, octave, mvuRight, mvDepth

// ---- double atan2 and cos in plain operations (fdlibm's atan with its published coefficients; cos as csrc/od_sincos.h) ----
TRI_FN double tri_fabs(double x) { return x < 0.0 ? -x : x; }
TRI_FN double tri_atan_pos(double x) {                           // atan for x >= 0 (or NaN)
    if (x != x) return x;
    if (x >= 7.378697629483821e19) return 1.57079632679489655800e+00 + 6.12323399573676603587e-17;   // 2^66
    int id; double hi, lo;
    if (x < 0.4375) { if (x < 1.862645149230957e-09) return x; id = -1; hi = 0.0; lo = 0.0; }
    else if (x < 1.1875) {
        if (x < 0.6875) { id = 0; hi = 4.63647609000806093515e-01; lo = 2.26987774529616870924e-17; x = (2.0 * x - 1.0) / (2.0 + x); }
        else { id = 1; hi = 7.85398163397448278999e-01; lo = 3.06161699786838301793e-17; x = (x - 1.0) / (x + 1.0); }
    } else if (x < 2.4375) { id = 2; hi = 9.82793723247329054082e-01; lo = 1.39033110312309984516e-17; x = (x - 1.5) / (1.0 + 1.5 * x); }
    else { id = 3; hi = 1.57079632679489655800e+00; lo = 6.12323399573676603587e-17; x = -1.0 / x; }
    const double z = x * x, w = z * z;
    const double s1 = z * (3.33333333333329318027e-01 + w * (1.42857142725034663711e-01 + w * (9.09088713343650656196e-02 +
                      w * (6.66107313738753120669e-02 + w * (4.97687799461593236017e-02 + w * 1.62858201153657823623e-02)))));
    const double s2 = w * (-1.99999999998764832476e-01 + w * (-1.11111104054623557880e-01 + w * (-7.69187620504482999495e-02 +
                      w * (-5.83357013379057348645e-02 + w * -3.65315727442169155270e-02))));
    if (id < 0) return x - x * (s1 + s2);
    return hi - ((x * (s1 + s2) - lo) - x);
}
TRI_FN double tri_atan2(double y, double x) {
    const double pi = 3.1415926535897931160E+00, pi_lo = 1.2246467991473531772E-16, pio2 = 1.57079632679489655800e+00;
    if (x != x || y != y) return x + y;
    if (y == 0.0) return x < 0.0 ? pi : y;                       // the sign of a zero y is kept for x >= 0; -0 with x < 0 reads as +pi here
    if (x == 0.0) return y < 0.0 ? -pio2 : pio2;
    const double z = tri_atan_pos(tri_fabs(y / x));
    if (x > 0.0) return y < 0.0 ? -z : z;
    return y < 0.0 ? (z - pi_lo) - pi : pi - (z - pi_lo);
}
TRI_FN double tri_cos(double xd) {                               // |xd| <= 2 pi: two-term reduction by pi/2, fdlibm kernels
    const double kd = __builtin_rint(xd * 0.63661977236758134308);
    const int k = (int)kd;
    double r = __builtin_fma(-kd, 1.57079632679489655800e+00, xd);
    r = __builtin_fma(-kd, 6.12323399573676603587e-17, r);
    const double z = r * r;
    double ps = __builtin_fma(z, 1.58969099521155010221e-10, -2.50507602534068634195e-08);
    ps = __builtin_fma(z, ps, 2.75573137070700676789e-06);
    ps = __builtin_fma(z, ps, -1.98412698298579493134e-04);
    ps = __builtin_fma(z, ps, 8.33333333332248946124e-03);
    ps = __builtin_fma(z, ps, -1.66666666666666324348e-01);
    const double S = __builtin_fma(z * r, ps, r);
    double pc = __builtin_fma(z, -1.13596475577881948265e-11, 2.08757232129817482790e-09);
    pc = __builtin_fma(z, pc, -2.75573143513906633035e-07);
    pc = __builtin_fma(z, pc, 2.48015872894767294178e-05);
    pc = __builtin_fma(z, pc, -1.38888888888741095749e-03);
    pc = __builtin_fma(z, pc, 4.16666666666666019037e-02);
    const double hz = 0.5 * z, w1 = 1.0 - hz;
    const double C = w1 + (((1.0 - w1) - hz) + z * z * pc);
    const double c0 = (k & 1) ? S : C;
    return ((k + 1) & 2) ? -c0 : c0;
}
// cos(2*atan2(mb/2, depth)) (:733, :736): mb/2 is a float quotient, the rest double, stored to float
TRI_FN float tri_cos_parallax_stereo(float mb, float depth) {
    const float half = mb / 2;
    return (float)tri_cos(2 * tri_atan2((double)half, (double)depth));
}

// ---- cv::Matx algebra as the reference's templates write it ----
TRI_FN float tri_dot3(const float* a, const float* b) { float s = 0; s += a[0] * b[0]; s += a[1] * b[1]; s += a[2] * b[2]; return s; }   // Matx::dot
TRI_FN double tri_norm3(const float* a) {                        // cv::norm(Matx31f): sqrt of a double sum
    double s = 0; s += (double)a[0] * (double)a[0]; s += (double)a[1] * (double)a[1]; s += (double)a[2] * (double)a[2];
    return __builtin_sqrt(s);
}
// Rwc * x with Rwc = Rcw.t(): row i of Rwc is column i of Rcw; Matx product, float accumulation from 0
TRI_FN void tri_rwc_mul(const float T[12], const float x[3], float out[3]) {
    for (int i = 0; i < 3; ++i) { float s = 0; s += T[i] * x[0]; s += T[4 + i] * x[1]; s += T[8 + i] * x[2]; out[i] = s; }
}

// One Hestenes rotation of columns p, q of a (and of v); false = already orthogonal to 2^-50 (nothing done)
TRI_FN bool tri_rotate(double* ap, double* aq, double* vp, double* vq) {
    double al = 0, be = 0, ga = 0;
    for (int k = 0; k < 4; ++k) { al += ap[k] * ap[k]; be += aq[k] * aq[k]; ga += ap[k] * aq[k]; }
    if (ga == 0.0 || ga * ga <= 7.888609052210118e-31 * (al * be)) return false;        // 2^-100
    const double zeta = (be - al) / (2.0 * ga);
    const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (tri_fabs(zeta) + __builtin_sqrt(1.0 + zeta * zeta));
    const double c = 1.0 / __builtin_sqrt(1.0 + t * t), s = c * t;
    for (int k = 0; k < 4; ++k) {
        const double x = ap[k], y = aq[k]; ap[k] = c * x - s * y; aq[k] = s * x + c * y;
        const double vx = vp[k], vy = vq[k]; vp[k] = c * vx - s * vy; vq[k] = s * vx + c * vy;
    }
    return true;
}
// The right singular vector of the smallest singular value of the row-major float32 4x4 A, rounded to float32; unit length up to that
// rounding, its sign whatever the rotations leave (x3D divides it out).  The columns and V are carried in double: with float32 columns
// the rounding of every rotation adds up to several times the error of an ordinary float32 SVD, in double only the last rounding is
// left.  Cyclic sweeps (0,1) (0,2) (0,3) (1,2) (1,3) (2,3), at most TRI_MAX_SWEEPS, ended by the first sweep without a rotation; the
// smallest column norm picks the vector, the lowest index on a tie.
TRI_FN void tri_null_vector(const float A[16], float xh[4]) {
    double a0[4], a1[4], a2[4], a3[4];
    double v0[4] = {1, 0, 0, 0}, v1[4] = {0, 1, 0, 0}, v2[4] = {0, 0, 1, 0}, v3[4] = {0, 0, 0, 1};
    for (int k = 0; k < 4; ++k) { a0[k] = (double)A[4 * k]; a1[k] = (double)A[4 * k + 1]; a2[k] = (double)A[4 * k + 2]; a3[k] = (double)A[4 * k + 3]; }
    for (int sweep = 0; sweep < TRI_MAX_SWEEPS; ++sweep) {
        bool rot = tri_rotate(a0, a1, v0, v1);
        rot = tri_rotate(a0, a2, v0, v2) || rot;
        rot = tri_rotate(a0, a3, v0, v3) || rot;
        rot = tri_rotate(a1, a2, v1, v2) || rot;
        rot = tri_rotate(a1, a3, v1, v3) || rot;
        rot = tri_rotate(a2, a3, v2, v3) || rot;
        if (!rot) break;
    }
    double n0 = 0, n1 = 0, n2 = 0, n3 = 0;
    for (int k = 0; k < 4; ++k) { n0 += a0[k] * a0[k]; n1 += a1[k] * a1[k]; n2 += a2[k] * a2[k]; n3 += a3[k] * a3[k]; }
    int j = 0; double nm = n0;
    if (n1 < nm) { nm = n1; j = 1; }
    if (n2 < nm) { nm = n2; j = 2; }
    if (n3 < nm) { nm = n3; j = 3; }
    for (int k = 0; k < 4; ++k) xh[k] = (float)(j == 0 ? v0[k] : j == 1 ? v1[k] : j == 2 ? v2[k] : v3[k]);
}

// KeyFrame::UnprojectStereo_ (KeyFrame.cc:1337-1352): mvKeys, not mvKeysUn; zeros for depth <= 0
TRI_FN void tri_unproject_stereo(const TriCam& K, const TriPose& P, const TriObs& o, float x3D[3]) {
    const float z = o.depth;
    if (z > 0) {
        const float x = (o.kx - K.cx) * z * K.invfx;
        const float y = (o.ky - K.cy) * z * K.invfy;
        const float xc[3] = {x, y, z};
        float r[3];
        tri_rwc_mul(P.T, xc, r);                                                // Twc_.get_minor<3,3>(0,0) * x3Dc
        x3D[0] = r[0] + P.ow[0]; x3D[1] = r[1] + P.ow[1]; x3D[2] = r[2] + P.ow[2];
    } else { x3D[0] = 0; x3D[1] = 0; x3D[2] = 0; }
}

// The reprojection gate of one KeyFrame (:813-842 / :846-868).  mbf is KeyFrame 1's in BOTH calls (:861 reads mpCurrentKeyFrame->mbf).
TRI_FN bool tri_reproj_fails(const TriCam& K, const TriPose& P, const TriObs& o, bool stereo, float mbf1, float sigma2, const float x3D[3], float z) {
    const float x = tri_dot3(P.T, x3D) + P.T[3];
    const float y = tri_dot3(P.T + 4, x3D) + P.T[7];
    const float invz = (float)(1.0 / (double)z);
    if (!stereo) {
        const float u = K.fx * x / z + K.cx, v = K.fy * y / z + K.cy;           // Pinhole::project
        const float ex = u - o.ux, ey = v - o.uy;
        return (double)(ex * ex + ey * ey) > 5.991 * (double)sigma2;
    }
    const float u = K.fx * x * invz + K.cx;
    const float ur = u - mbf1 * invz;
    const float v = K.fy * y * invz + K.cy;
    const float ex = u - o.ux, ey = v - o.uy, er = ur - o.uright;
    return (double)(ex * ex + ey * ey + er * er) > 7.8 * (double)sigma2;
}

// One match of LocalMapping.cc:611-892.  sf* = mvScaleFactors, ls* = mvLevelSigma2 (nlevels entries each); ratio_factor = 1.5f *
// mfScaleFactor; th_far <= 0 turns the far-point test off.  Returns the reason; x3D is written on success (and holds the rejected
// candidate or zeros otherwise).  xh_out, where not NULL, receives x3D_h of the triangulated branch (the host tests read it).
TRI_FN int tri_one_match(const TriCam& K1, const TriCam& K2, float mb1, float mbf1, float mb2, const TriPose& P1, const TriPose& P2,
                         const TriObs& o1, const TriObs& o2, const float* sf1, const float* ls1, const float* sf2, const float* ls2,
                         int nlevels, float ratio_factor, float th_far, float x3D[3], float* xh_out = nullptr) {
    x3D[0] = 0; x3D[1] = 0; x3D[2] = 0;
    if ((unsigned)o1.octave >= (unsigned)nlevels || (unsigned)o2.octave >= (unsigned)nlevels) return TRI_BAD_OCTAVE;
    const bool st1 = o1.uright >= 0, st2 = o2.uright >= 0;
    const float xn1[3] = {(o1.ux - K1.cx) / K1.fx, (o1.uy - K1.cy) / K1.fy, 1.f};   // Pinhole::unproject
    const float xn2[3] = {(o2.ux - K2.cx) / K2.fx, (o2.uy - K2.cy) / K2.fy, 1.f};
    float ray1[3], ray2[3];
    tri_rwc_mul(P1.T, xn1, ray1); tri_rwc_mul(P2.T, xn2, ray2);
    const float cosRays = (float)((double)tri_dot3(ray1, ray2) / (tri_norm3(ray1) * tri_norm3(ray2)));
    float cosSt = cosRays + 1, cosSt1 = cosSt, cosSt2 = cosSt;
    if (st1) cosSt1 = tri_cos_parallax_stereo(mb1, o1.depth);
    else if (st2) cosSt2 = tri_cos_parallax_stereo(mb2, o2.depth);
    cosSt = cosSt2 < cosSt1 ? cosSt2 : cosSt1;                                  // std::min(cosSt1, cosSt2)
    int how;
    if (cosRays < cosSt && cosRays > 0 && (st1 || st2 || (double)cosRays < 0.9998)) {
        float A[16];
        for (int c = 0; c < 4; ++c) {
            A[c] = xn1[0] * P1.T[8 + c] - P1.T[c];
            A[4 + c] = xn1[1] * P1.T[8 + c] - P1.T[4 + c];
            A[8 + c] = xn2[0] * P2.T[8 + c] - P2.T[c];
            A[12 + c] = xn2[1] * P2.T[8 + c] - P2.T[4 + c];
        }
        float xh[4];
        tri_null_vector(A, xh);
        if (xh_out) { xh_out[0] = xh[0]; xh_out[1] = xh[1]; xh_out[2] = xh[2]; xh_out[3] = xh[3]; }
        if (xh[3] == 0) return TRI_W_ZERO;
        x3D[0] = xh[0] / xh[3]; x3D[1] = xh[1] / xh[3]; x3D[2] = xh[2] / xh[3];
        how = TRI_OK_TRIANGULATED;
    } else if (st1 && cosSt1 < cosSt2) { tri_unproject_stereo(K1, P1, o1, x3D); how = TRI_OK_STEREO1; }
    else if (st2 && cosSt2 < cosSt1) { tri_unproject_stereo(K2, P2, o2, x3D); how = TRI_OK_STEREO2; }
    else return TRI_LOW_PARALLAX;
    const float z1 = tri_dot3(P1.T + 8, x3D) + P1.T[11];
    if (z1 <= 0) return TRI_BEHIND_1;
    const float z2 = tri_dot3(P2.T + 8, x3D) + P2.T[11];
    if (z2 <= 0) return TRI_BEHIND_2;
    if (tri_reproj_fails(K1, P1, o1, st1, mbf1, ls1[o1.octave], x3D, z1)) return TRI_CHI2_1;
    if (tri_reproj_fails(K2, P2, o2, st2, mbf1, ls2[o2.octave], x3D, z2)) return TRI_CHI2_2;
    const float n1[3] = {x3D[0] - P1.ow[0], x3D[1] - P1.ow[1], x3D[2] - P1.ow[2]};
    const float n2[3] = {x3D[0] - P2.ow[0], x3D[1] - P2.ow[1], x3D[2] - P2.ow[2]};
    const float dist1 = (float)tri_norm3(n1), dist2 = (float)tri_norm3(n2);
    if (dist1 == 0 || dist2 == 0) return TRI_DIST_ZERO;
    if (th_far > 0 && (dist1 >= th_far || dist2 >= th_far)) return TRI_FAR;
    const float ratioDist = dist2 / dist1;
    const float ratioOctave = sf1[o1.octave] / sf2[o2.octave];
    if (ratioDist * ratio_factor < ratioOctave || ratioDist > ratioOctave * ratio_factor) return TRI_SCALE;
    return how;
}
