// orbm_poseopt.h -- the arithmetic of Optimizer::PoseOptimization(Frame*) (Optimizer.cc:943-1286, !mpCamera2), once, for both sides:
// k_pose_opt (orbm_kernels.hip.h) compiles it for the device and tests/poseopt_header.cpp for the host.  Plain C++: no HIP, no <cmath>;
// the square root is the compiler's builtin (IEEE, correctly rounded on both sides), sine and cosine are the fdlibm kernels below, and the
// build passes -ffp-contract=off, so both sides execute the same IEEE double operations in the same order.
//
// What is restated (file:line in the reference tree):
//   edges      one per slot with a MapPoint, mono where mvuRight < 0, stereo otherwise (Optimizer.cc:998-1083).  Information =
//              mvInvLevelSigma2[octave] * I, Huber delta (float)sqrt(5.991) / (float)sqrt(7.815) widened to double, dsqr = delta * delta.
//   mono       error = obs - (fx * x / z + cx, fy * y / z + cy), in that order (Pinhole.cpp:66-73); J = -projectJac * SE3deriv
//              (OptimizableTypes.cpp:51-65, Pinhole.cpp:151-162).
//   stereo     cam_project's `const float invz = 1.0f / trans_xyz[2]` (types_six_dof_expmap.cpp:339-346): the FLOAT invz, here the double
//              quotient rounded to float as C++ evaluates that line; the Jacobian (:375-404) uses the double invz.  Both kept as written.
//   form       with a kernel b -= rho[1] * J^T Omega e, H += J^T (rho[1] * Omega) J, rho[2] unused, the chi sum adds rho[0]
//              (base_unary_edge.hpp:43-72, robust_kernel_impl.cpp:78-91); without one the plain forms.
//   LM         optimization_algorithm_levenberg.cpp:61-194: lambda = 1e-5 * max|H_jj| and ni = 2 at iteration 0 only; per trial LDLT of
//              H + lambda I (not positive => tempChi = DBL_MAX and x keeps its last value), oplus = exp(x) * estimate (se3quat.h:223-257,
//              both theta branches), rho = (currentChi - tempChi) / (sum x_j (lambda x_j + b_j) + 1e-3), accept iff rho > 0 and tempChi
//              finite, alpha = 1 - (2 rho - 1)^3 clamped to [1/3, 2/3]; on reject lambda *= ni, ni *= 2; loop while rho < 0 and qmax < 10;
//              qmax == 10 or rho == 0 terminates; (iniChi - currentChi) * 1e3 < iniChi three times in a row terminates; optimize(10)
//              stops at the first result that is not OK (sparse_optimizer.cpp:354-419).
//   rounds     Optimizer.cc:1173-1275.  ROUND-RESTART RULE: every round starts from the INPUT pose (mTcw is written after the last
//              round only); the rounds differ in their active set and, in round 3, in having no kernel.  After each round every edge is
//              classified: `const float chi2 = e->chi2(); chi2 > 5.991f / 7.815f`, i.e. the chi2 rounded to float against the float
//              threshold, strictly.  An edge flagged as an outlier is recomputed at the round's final pose first.  STALE-ERROR RULE: an
//              inlier edge is read as the last computeActiveErrors left it -- after a rejected last trial that is the error at the
//              REJECTED pose, pop() restores the estimate and not the errors.  A round whose active set is empty optimises nothing
//              (no active vertex: optimize() returns at once) and classifies at the input pose.  Fewer than 10 edges in all: one
//              round.  Fewer than 3: nothing runs, the flags are cleared, the pose is not touched, the result is 0.
//
// What differs from g2o, inside the tolerance DESIGN section 8 states: the pose is held as a 3x4 double matrix, not as quaternion +
// vector.  Where g2o's quaternion makes a matrix a rotation -- SE3Quat(R, t) of the float input pose and Quaterniond(R) of exp()'s R,
// whose small-theta form I + W + W^2 is no rotation -- the same round trip is made here (po_rotation_roundtrip); products and map() then
// differ from the quaternion forms by rounding only.  LDLT runs without pivoting, (2 rho - 1)^3 and theta^3 are products.
//
// REDUCTION ORDER, part of the contract (the sums decide the bits): slot s belongs to thread s % 256 of the frame's workgroup; a thread
// adds its slots s = t, t + 256, ... in ascending order into 28 partial sums (the upper triangle of H row by row, b, chi), starting from
// +0; the 64 lanes of a wave combine by an xor butterfly with masks 32, 16, 8, 4, 2, 1 (v = v + other; the add is commutative, so every
// lane holds the same bits); the four wave sums are added in wave order, ((w0 + w1) + w2) + w3.  PoCpuReduce below replays that order
// with loops; the device context in orbm_kernels.hip.h executes it.
#pragma once
#ifndef PO_FN
#define PO_FN static inline
#endif

#define PO_THREADS 256
#define PO_NACC 28                                     // 21 (upper triangle of H) + 6 (b) + 1 (chi)
#define PO_DBL_MAX 1.7976931348623157e308
#define PO_DELTA_MONO   ((double)2.4476518630981445f)  // (float)sqrt(5.991), widened
#define PO_DELTA_STEREO ((double)2.7955322265625f)     // (float)sqrt(7.815), widened
#define PO_CHI2_MONO 5.991f
#define PO_CHI2_STEREO 7.815f
enum { PO_INLIER = 0, PO_OUTLIER = 1, PO_NONE = 2 };   // per-slot state: an inlier is active (level 0), an outlier is not (level 1)

struct PoCam { double fx, fy, cx, cy, bf; };
struct PoEdge { double u, v, ur, X, Y, Z, w; bool stereo; };   // obs, Xw and invSigma2: floats widened

// the edge of one slot that holds a MapPoint (Optimizer.cc:1008-1082); false = the slot is treated as NULL: an octave outside
// [0, nlevels), where the reference would read past mvInvLevelSigma2.  uright == nullptr makes the edge mono.
PO_FN bool po_make_edge(float x, float y, int octave, const float* uright, const float* Xw, const float* ils2, int nlevels, PoEdge& e) {
    if (octave < 0 || octave >= nlevels) return false;
    e.u = (double)x; e.v = (double)y;
    e.stereo = uright && !(*uright < 0);
    e.ur = e.stereo ? (double)*uright : 0.0;
    e.X = (double)Xw[0]; e.Y = (double)Xw[1]; e.Z = (double)Xw[2];
    e.w = (double)ils2[octave];
    return true;
}

// sin and cos of theta >= 0: Cody-Waite reduction by pi/2 in two terms and the fdlibm kernel polynomials on |r| <= pi/4, as od_sincos.h.
// An LM step's theta is far below 1; the reduction stays within an ulp of double for theta up to a few thousand and degrades slowly
// beyond, the same on both sides.
PO_FN void po_sincos(double x, double* sn, double* cs) {
    const double kd = __builtin_rint(x * 0.63661977236758134308);
    const long long k = (long long)kd;
    double r = __builtin_fma(-kd, 1.57079632679489655800e+00, x);
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
    const double Cc = w1 + (((1.0 - w1) - hz) + z * z * pc);
    const bool sw = (k & 1) != 0;
    const double s0 = sw ? Cc : S, c0 = sw ? S : Cc;
    *sn = (k & 2) ? -s0 : s0;
    *cs = ((k + 1) & 2) ? -c0 : c0;
}

// R (row-major 3x3) -> Eigen's Quaterniond(R) -> normalize -> toRotationMatrix(): what SE3Quat's constructors do to a matrix
PO_FN void po_rotation_roundtrip(double R[9]) {
    double qw, qx, qy, qz;
    double t = R[0] + R[4] + R[8];
    if (t > 0.0) {
        t = __builtin_sqrt(t + 1.0);
        qw = 0.5 * t;
        t = 0.5 / t;
        qx = (R[7] - R[5]) * t; qy = (R[2] - R[6]) * t; qz = (R[3] - R[1]) * t;
    } else {
        int i = 0;
        if (R[4] > R[0]) i = 1;
        if (R[8] > R[4 * i]) i = 2;
        const int j = (i + 1) % 3, k = (j + 1) % 3;
        double q[3];
        t = __builtin_sqrt(R[4 * i] - R[4 * j] - R[4 * k] + 1.0);
        q[i] = 0.5 * t;
        t = 0.5 / t;
        qw = (R[3 * k + j] - R[3 * j + k]) * t;
        q[j] = (R[3 * j + i] + R[3 * i + j]) * t;
        q[k] = (R[3 * k + i] + R[3 * i + k]) * t;
        qx = q[0]; qy = q[1]; qz = q[2];
    }
    const double n = __builtin_sqrt(((qx * qx + qy * qy) + qz * qz) + qw * qw);
    qx = qx / n; qy = qy / n; qz = qz / n; qw = qw / n;
    const double tx = 2.0 * qx, ty = 2.0 * qy, tz = 2.0 * qz;
    const double twx = tx * qw, twy = ty * qw, twz = tz * qw, txx = tx * qx, txy = ty * qx, txz = tz * qx, tyy = ty * qy, tyz = tz * qy, tzz = tz * qz;
    R[0] = 1.0 - (tyy + tzz); R[1] = txy - twz; R[2] = txz + twy;
    R[3] = txy + twz; R[4] = 1.0 - (txx + tzz); R[5] = tyz - twx;
    R[6] = txz - twy; R[7] = tyz + twx; R[8] = 1.0 - (txx + tyy);
}

// the float [Rcw | tcw] row -> the estimate: Converter::toSE3Quat (Converter.cc:42-55)
PO_FN void po_pose_from_float(const float* tcw12, double T[12]) {
    double R[9];
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) R[3 * r + c] = (double)tcw12[4 * r + c];
    po_rotation_roundtrip(R);
    for (int r = 0; r < 3; ++r) { T[4 * r] = R[3 * r]; T[4 * r + 1] = R[3 * r + 1]; T[4 * r + 2] = R[3 * r + 2]; T[4 * r + 3] = (double)tcw12[4 * r + 3]; }
}

// Tn = SE3Quat::exp(x) * T (se3quat.h:223-257, VertexSE3Expmap::oplusImpl); x = (omega, upsilon)
PO_FN void po_oplus(const double x[6], const double T[12], double Tn[12]) {
    const double wx = x[0], wy = x[1], wz = x[2];
    const double theta = __builtin_sqrt((wx * wx + wy * wy) + wz * wz);
    const double W[9] = {0.0, -wz, wy, wz, 0.0, -wx, -wy, wx, 0.0};
    double W2[9];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) W2[3 * r + c] = (W[3 * r] * W[c] + W[3 * r + 1] * W[3 + c]) + W[3 * r + 2] * W[6 + c];
    double R[9], V[9];
    if (theta < 0.00001) {
        for (int i = 0; i < 9; ++i) { R[i] = ((i % 4 == 0 ? 1.0 : 0.0) + W[i]) + W2[i]; V[i] = R[i]; }
    } else {
        double sn, cs;
        po_sincos(theta, &sn, &cs);
        const double a = sn / theta, b = (1.0 - cs) / (theta * theta), c = (theta - sn) / ((theta * theta) * theta);
        for (int i = 0; i < 9; ++i) {
            const double id = i % 4 == 0 ? 1.0 : 0.0;
            R[i] = (id + a * W[i]) + b * W2[i];
            V[i] = (id + b * W[i]) + c * W2[i];
        }
    }
    double te[3];
    for (int r = 0; r < 3; ++r) te[r] = (V[3 * r] * x[3] + V[3 * r + 1] * x[4]) + V[3 * r + 2] * x[5];
    po_rotation_roundtrip(R);
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) Tn[4 * r + c] = (R[3 * r] * T[c] + R[3 * r + 1] * T[4 + c]) + R[3 * r + 2] * T[8 + c];
        Tn[4 * r + 3] = te[r] + ((R[3 * r] * T[3] + R[3 * r + 1] * T[7]) + R[3 * r + 2] * T[11]);
    }
}

// the edge's error at pose T and its chi2 = e . (Omega e); returns the camera-frame point in xc
PO_FN double po_edge_error(const PoCam& C, const double T[12], const PoEdge& e, double err[3], double xc[3]) {
    const double x = ((T[0] * e.X + T[1] * e.Y) + T[2] * e.Z) + T[3];
    const double y = ((T[4] * e.X + T[5] * e.Y) + T[6] * e.Z) + T[7];
    const double z = ((T[8] * e.X + T[9] * e.Y) + T[10] * e.Z) + T[11];
    xc[0] = x; xc[1] = y; xc[2] = z;
    double chi;
    if (!e.stereo) {
        err[0] = e.u - (C.fx * x / z + C.cx);
        err[1] = e.v - (C.fy * y / z + C.cy);
        err[2] = 0.0;
        chi = err[0] * (e.w * err[0]) + err[1] * (e.w * err[1]);
    } else {
        const double invz = (double)(float)(1.0 / z);                         // const float invz = 1.0f / trans_xyz[2]
        const double p0 = x * invz * C.fx + C.cx;
        err[0] = e.u - p0;
        err[1] = e.v - (y * invz * C.fy + C.cy);
        err[2] = e.ur - (p0 - C.bf * invz);
        chi = (err[0] * (e.w * err[0]) + err[1] * (e.w * err[1])) + err[2] * (e.w * err[2]);
    }
    return chi;
}

PO_FN double po_edge_chi2(const PoCam& C, const double T[12], const PoEdge& e) {
    double err[3], xc[3];
    return po_edge_error(C, T, e, err, xc);
}

// rho[0] and rho[1] of RobustKernelHuber::robustify, or the plain (chi2, 1) without a kernel
PO_FN void po_robustify(double chi2, bool stereo, bool kernel, double* rho0, double* rho1) {
    const double delta = stereo ? PO_DELTA_STEREO : PO_DELTA_MONO, dsqr = delta * delta;
    if (!kernel || chi2 <= dsqr) { *rho0 = chi2; *rho1 = 1.0; return; }
    const double s = __builtin_sqrt(chi2);
    *rho0 = 2 * s * delta - dsqr;
    *rho1 = delta / s;
}

// the robust chi of one active edge at T: what computeActiveErrors + activeRobustChi2 add for it
PO_FN double po_edge_chi(const PoCam& C, const double T[12], const PoEdge& e, bool kernel) {
    double r0, r1;
    po_robustify(po_edge_chi2(C, T, e), e.stereo, kernel, &r0, &r1);
    return r0;
}

// one active edge's contribution to acc[28] at T: linearizeOplus + constructQuadraticForm, and its robust chi
PO_FN void po_edge_system(const PoCam& C, const double T[12], const PoEdge& e, bool kernel, double acc[PO_NACC]) {
    double err[3], xc[3], J[3][6], r0, r1;
    const double chi2 = po_edge_error(C, T, e, err, xc);
    po_robustify(chi2, e.stereo, kernel, &r0, &r1);
    const double x = xc[0], y = xc[1], z = xc[2];
    int rows;
    if (!e.stereo) {
        rows = 2;
        const double j00 = C.fx / z, j02 = -C.fx * x / (z * z), j11 = C.fy / z, j12 = -C.fy * y / (z * z);
        J[0][0] = -(j02 * y); J[0][1] = -(j00 * z + j02 * -x); J[0][2] = -(j00 * -y); J[0][3] = -j00; J[0][4] = -0.0; J[0][5] = -j02;
        J[1][0] = -(j11 * -z + j12 * y); J[1][1] = -(j12 * -x); J[1][2] = -(j11 * x); J[1][3] = -0.0; J[1][4] = -j11; J[1][5] = -j12;
        for (int c = 0; c < 6; ++c) J[2][c] = 0.0;
    } else {
        rows = 3;
        const double invz = 1.0 / z, invz_2 = invz * invz;
        J[0][0] = x * y * invz_2 * C.fx; J[0][1] = -(1 + (x * x * invz_2)) * C.fx; J[0][2] = y * invz * C.fx;
        J[0][3] = -invz * C.fx; J[0][4] = 0; J[0][5] = x * invz_2 * C.fx;
        J[1][0] = (1 + y * y * invz_2) * C.fy; J[1][1] = -x * y * invz_2 * C.fy; J[1][2] = -x * invz * C.fy;
        J[1][3] = 0; J[1][4] = -invz * C.fy; J[1][5] = y * invz_2 * C.fy;
        J[2][0] = J[0][0] - C.bf * y * invz_2; J[2][1] = J[0][1] + C.bf * x * invz_2; J[2][2] = J[0][2];
        J[2][3] = J[0][3]; J[2][4] = 0; J[2][5] = J[0][5] - C.bf * invz_2;
    }
    const double wo = r1 * e.w;                                               // robustInformation: rho[1] * Omega
    int k = 0;
    for (int a = 0; a < 6; ++a)
        for (int b = a; b < 6; ++b, ++k) {
            double s = J[0][a] * wo * J[0][b] + J[1][a] * wo * J[1][b];
            if (rows == 3) s = s + J[2][a] * wo * J[2][b];
            acc[k] = acc[k] + s;
        }
    for (int a = 0; a < 6; ++a) {
        double s = J[0][a] * (e.w * err[0]) + J[1][a] * (e.w * err[1]);
        if (rows == 3) s = s + J[2][a] * (e.w * err[2]);
        acc[21 + a] = acc[21 + a] - r1 * s;
    }
    acc[27] = acc[27] + r0;
}

// the classification of Optimizer.cc:1184-1271 for one edge: chi2 of the stored error (at Terr for an inlier, recomputed at T for an
// outlier), rounded to float, strictly above the float threshold
PO_FN int po_edge_classify(const PoCam& C, const double Terr[12], const double T[12], const PoEdge& e, int state) {
    const float chi2 = (float)po_edge_chi2(C, state == PO_OUTLIER ? T : Terr, e);
    return chi2 > (e.stereo ? PO_CHI2_STEREO : PO_CHI2_MONO) ? PO_OUTLIER : PO_INLIER;
}

// (H + lambda I) x = b by LDLT without pivoting on the upper triangle h[21]; false (x untouched) unless every pivot is > 0
PO_FN bool po_solve6(const double h[21], double lambda, const double b[6], double x[6]) {
    double A[6][6], L[6][6], D[6], y[6];
    int k = 0;
    for (int r = 0; r < 6; ++r)
        for (int c = r; c < 6; ++c, ++k) { A[r][c] = h[k]; A[c][r] = h[k]; }
    for (int r = 0; r < 6; ++r) A[r][r] = A[r][r] + lambda;
    for (int j = 0; j < 6; ++j) {
        double d = A[j][j];
        for (int p = 0; p < j; ++p) d = d - L[j][p] * L[j][p] * D[p];
        if (!(d > 0.0)) return false;
        D[j] = d;
        for (int i = j + 1; i < 6; ++i) {
            double s = A[i][j];
            for (int p = 0; p < j; ++p) s = s - L[i][p] * L[j][p] * D[p];
            L[i][j] = s / d;
        }
    }
    for (int i = 0; i < 6; ++i) {
        double s = b[i];
        for (int p = 0; p < i; ++p) s = s - L[i][p] * y[p];
        y[i] = s;
    }
    for (int i = 5; i >= 0; --i) {
        double s = y[i] / D[i];
        for (int p = i + 1; p < 6; ++p) s = s - L[p][i] * x[p];
        x[i] = s;
    }
    return true;
}

PO_FN bool po_finite(double v) { return v == v && v <= PO_DBL_MAX && v >= -PO_DBL_MAX; }

// One optimize(10) over the context's active edges, from T (in/out).  Terr receives the pose of the last computeActiveErrors.
// x is the solver's solution vector: it outlives the call (Solver::resizeVector keeps the allocation between optimize() calls,
// solver.cpp:46-69) and is only read when an LDLT was not positive.
// Ctx: void system(const double T[12], bool kernel, double acc[28]);  double chi(const double T[12], bool kernel).
template <class Ctx>
PO_FN void po_optimize10(Ctx& ctx, bool kernel, double T[12], double Terr[12], double x[6]) {
    double lambda = 0.0, ni = 2.0;
    int nBad = 0;
    for (int it = 0; it < 10; ++it) {
        double acc[PO_NACC];
        ctx.system(T, kernel, acc);
        for (int i = 0; i < 12; ++i) Terr[i] = T[i];
        double currentChi = acc[27];
        const double iniChi = currentChi;
        const double* b = acc + 21;
        if (it == 0) {
            double md = 0.0;
            for (int j = 0, k = 0; j < 6; k += 6 - j, ++j) { const double d = acc[k] < 0.0 ? -acc[k] : acc[k]; md = d > md ? d : md; }
            lambda = 1e-5 * md; ni = 2.0; nBad = 0;
        }
        double rho = 0.0;
        int qmax = 0;
        do {
            const bool ok = po_solve6(acc, lambda, b, x);
            double Tn[12];
            po_oplus(x, T, Tn);
            double tempChi = ctx.chi(Tn, kernel);
            for (int i = 0; i < 12; ++i) Terr[i] = Tn[i];
            if (!ok) tempChi = PO_DBL_MAX;
            rho = currentChi - tempChi;
            double scale = 0.0;
            for (int j = 0; j < 6; ++j) scale = scale + x[j] * (lambda * x[j] + b[j]);
            scale = scale + 1e-3;
            rho = rho / scale;
            if (rho > 0.0 && po_finite(tempChi)) {
                const double q = 2 * rho - 1;
                double alpha = 1. - (q * q) * q;
                alpha = alpha < 2. / 3. ? alpha : 2. / 3.;
                const double sf = 1. / 3. > alpha ? 1. / 3. : alpha;
                lambda = lambda * sf; ni = 2.0; currentChi = tempChi;
                for (int i = 0; i < 12; ++i) T[i] = Tn[i];
            } else {
                lambda = lambda * ni; ni = ni * 2.0;
            }
            ++qmax;
        } while (rho < 0.0 && qmax < 10);
        if (qmax == 10 || rho == 0.0) break;
        if ((iniChi - currentChi) * 1e3 < iniChi) ++nBad; else nBad = 0;
        if (nBad >= 3) break;
    }
}

// The four rounds.  The caller has counted nCorr >= 3 edges and set every edge's state to PO_INLIER.  T0 = the estimate of the input
// pose (po_pose_from_float).  Ctx adds: int classify(const double Terr[12], const double T[12]) -- applies po_edge_classify to every
// edge, stores the new states and returns the number of outliers.  Returns nInitialCorrespondences - nBad; Tout = the last round's pose.
template <class Ctx>
PO_FN int po_four_rounds(Ctx& ctx, int nCorr, const double T0[12], double Tout[12]) {
    int nBad = 0;
    double x[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};                           // one solution vector for the four rounds (the reference's starts undefined; 0 here)
    for (int round = 0; round < 4; ++round) {
        double T[12], Terr[12];
        for (int i = 0; i < 12; ++i) { T[i] = T0[i]; Terr[i] = T0[i]; }
        if (nCorr - nBad > 0) po_optimize10(ctx, round < 3, T, Terr, x);
        nBad = ctx.classify(Terr, T);
        for (int i = 0; i < 12; ++i) Tout[i] = T[i];
        if (nCorr < 10) break;
    }
    return nCorr - nBad;
}

// ---- the host replay of the reduction order (tests, and the host timing of tools/pose_optimization_batch.py) ----
#ifndef __HIP_DEVICE_COMPILE__
struct PoCpuReduce {
    PoCam C;
    int n;                        // slots
    const PoEdge* e;              // [n]
    unsigned char* state;         // [n] PO_INLIER / PO_OUTLIER / PO_NONE

    void combine(double (*part)[PO_NACC], int nacc, double* out) const {   // part[256][28] -> butterfly per wave, waves in order
        for (int a = 0; a < nacc; ++a) {
            double w[4];
            for (int wv = 0; wv < 4; ++wv) {
                double v[64], o[64];
                for (int l = 0; l < 64; ++l) v[l] = part[wv * 64 + l][a];
                for (int m = 32; m >= 1; m >>= 1) {
                    for (int l = 0; l < 64; ++l) o[l] = v[l] + v[l ^ m];
                    for (int l = 0; l < 64; ++l) v[l] = o[l];
                }
                w[wv] = v[0];
            }
            out[a] = ((w[0] + w[1]) + w[2]) + w[3];
        }
    }
    void system(const double T[12], bool kernel, double acc[PO_NACC]) const {
        static thread_local double part[PO_THREADS][PO_NACC];
        for (int t = 0; t < PO_THREADS; ++t) {
            for (int a = 0; a < PO_NACC; ++a) part[t][a] = 0.0;
            for (int s = t; s < n; s += PO_THREADS)
                if (state[s] == PO_INLIER) po_edge_system(C, T, e[s], kernel, part[t]);
        }
        combine(part, PO_NACC, acc);
    }
    double chi(const double T[12], bool kernel) const {
        static thread_local double part[PO_THREADS][PO_NACC];
        for (int t = 0; t < PO_THREADS; ++t) {
            part[t][0] = 0.0;
            for (int s = t; s < n; s += PO_THREADS)
                if (state[s] == PO_INLIER) part[t][0] = part[t][0] + po_edge_chi(C, T, e[s], kernel);
        }
        double out;
        combine(part, 1, &out);
        return out;
    }
    int classify(const double Terr[12], const double T[12]) const {
        int nBad = 0;
        for (int s = 0; s < n; ++s)
            if (state[s] != PO_NONE) { state[s] = (unsigned char)po_edge_classify(C, Terr, T, e[s], state[s]); nBad += state[s] == PO_OUTLIER; }
        return nBad;
    }
};
#endif
