// screen_rects.h — the per-frame table of screen boxes of a one-body scene's leaf references (DESIGN.md §3 "Screen boxes of the primary packets").
// A frame's primary rays come from one camera: the ray k_raygen builds at the sample position (sx, sy) can be accepted by RE:42-75 for triangle t only
// if (sx, sy) lies inside t's ENTRY -- the screen bounding box of the points within delta(t) of t, rounded outwards to 1/16 pixel.  k_packet #0 of a camera
// frame compares the entries of a leaf with the screen rectangle of its packet (wave-uniform) and gives no triangle step to a triangle whose entry misses it.
// Everything here is evaluated in double from the binary32 inputs, by the same functions on the host and on the device (-ffp-contract=off on both sides):
// tests/screen_rects compares the table entry by entry.
#pragma once
#include "xrt_core.h"

namespace xrt {

constexpr unsigned SCR_NO_CULL = 0xffffffffu;   // both words: "the proof is not available for this triangle", the walk tests it as before
constexpr int SCR_UNITS = 16, SCR_BIAS = 8, SCR_MAX = 65534;   // a field: floor / ceil of 16 x + 8, clamped to 0 .. 65534 (x: screen coordinate in pixels)
constexpr int SCR_MAX_EXTENT = 4000;                           // widest / highest viewport the fields hold (with the sample offsets and the bias)
struct ScrEntry { unsigned x, y; };                            // x0 | x1 << 16, y0 | y1 << 16

// What a frame contributes: the exact map of the body's space to the screen that the binary32 rays approximate, and how well they do.
struct ScreenXf {
    double F[16];              // body space -> clip space, row vectors: the inverse of B = g.m x invWorld (what unproject and the body transform apply)
    double E[3];               // the eye in the body's space: every exact ray of the frame passes through it
    double vpX, vpY, vpW, vpH;
    double dN;                 // >= |O - E| for every ray origin O of the frame (binary32, body space)
    double epsO;               // >= |O - O*|: the binary32 origin against the exact one of the same sample position
    double epsT;               // >= |D / |D| - d*|: the binary32 direction against the exact one
    double fx, fy, fw;         // lengths of the three-vectors (F[0], F[4], F[8]), (F[1], F[5], F[9]), (F[3], F[7], F[11]): how fast clip x, y and w change with the point
    double resid;              // |B x F - 1|, largest element: how far F is from the inverse (it enters every entry's padding)
    int ok;                    // 0: no entry of this frame may cull
    int why;                   // ... and the check that said so (diagnostics: tests/screen_rects prints it)
};

// B^-1 by Gauss-Jordan with partial pivoting; false when B is singular to working precision.  Every index is a constant once the loops are unrolled (the
// pivot row comes up through conditional swaps): on the device the matrix stays in registers.
XRT_HD bool scr_invert4(const double *B, double *F) {
    double a[4][8];
#pragma unroll
    for (int i = 0; i < 4; i++) {
#pragma unroll
        for (int j = 0; j < 4; j++) { a[i][j] = B[4 * i + j]; a[i][4 + j] = i == j ? 1.0 : 0.0; }
    }
    bool ok = true;
#pragma unroll
    for (int c = 0; c < 4; c++) {
#pragma unroll
        for (int r = c + 1; r < 4; r++) {
            const bool sw = fabs(a[r][c]) > fabs(a[c][c]);
#pragma unroll
            for (int j = 0; j < 8; j++) { const double t = a[r][j], w = a[c][j]; a[c][j] = sw ? t : w; a[r][j] = sw ? w : t; }
        }
        ok = ok && fabs(a[c][c]) > 0.0;
        const double inv = 1.0 / a[c][c];
#pragma unroll
        for (int j = 0; j < 8; j++) a[c][j] *= inv;
#pragma unroll
        for (int r = 0; r < 4; r++) {
            if (r == c) continue;
            const double f = a[r][c];
#pragma unroll
            for (int j = 0; j < 8; j++) a[r][j] -= f * a[c][j];
        }
    }
#pragma unroll
    for (int i = 0; i < 4; i++) {
#pragma unroll
        for (int j = 0; j < 4; j++) F[4 * i + j] = a[i][4 + j];
    }
    return ok;
}
XRT_HD void scr_mul4(const double *a, const double *b, double *r) {
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) r[4 * i + j] = a[4 * i] * b[j] + a[4 * i + 1] * b[4 + j] + a[4 * i + 2] * b[8 + j] + a[4 * i + 3] * b[12 + j];
}
// (X, Y, Z, 1) x M, dehomogenised; false when w vanishes
XRT_HD bool scr_point(const double *M, double X, double Y, double Z, double *p) {
    double v[4];
    for (int j = 0; j < 4; j++) v[j] = X * M[j] + Y * M[4 + j] + Z * M[8 + j] + M[12 + j];
    if (!(fabs(v[3]) > 1e-300)) return false;
    p[0] = v[0] / v[3]; p[1] = v[1] / v[3]; p[2] = v[2] / v[3];
    return true;
}

// The frame's part.  invWorld: the body's ObjRec::invWorld as traverse.h lane_begin applies it (Vector3.Transform: its fourth column is not read).
// The error terms bound k_raygen's binary32 arithmetic (unproject twice, normalize) and lane_begin's (transform twice, normalize) over every sample
// position of the viewport; the derivation is DESIGN.md's.  u = 2^-24.
XRT_HD void make_screen_xf(const RayGenParams &g, const float *invWorld, ScreenXf &X) {
    const double u = 5.9604644775390625e-8;
    X.ok = 0; X.why = 1; X.resid = 0.0;
    X.vpX = g.vpX; X.vpY = g.vpY; X.vpW = g.vpW; X.vpH = g.vpH;
    double G[16], IW[16], B[16];
#pragma unroll
    for (int i = 0; i < 16; i++) { G[i] = g.m[i]; IW[i] = invWorld[i]; }
    IW[3] = 0.0; IW[7] = 0.0; IW[11] = 0.0; IW[15] = 1.0;
    scr_mul4(G, IW, B);
    if (!scr_invert4(B, X.F)) return;
    X.why = 2;
    {   // the inverse is one: B x F = 1 to 1e-6 (what is left widens every entry, screen_entry)
        double I[16];
        scr_mul4(B, X.F, I);
#pragma unroll
        for (int i = 0; i < 16; i++) { const double d = fabs(I[i] - ((i % 5) == 0 ? 1.0 : 0.0)); if (!(d <= 1e-6)) return; X.resid = fmax(X.resid, d); }
    }
    X.why = 3;
    // the eye: every (X, Y, Z, 1) x B lies on the line through (X, Y, 0, 1) x B and row 2 of B
    if (!(fabs(B[11]) > 1e-9 * (fabs(B[8]) + fabs(B[9]) + fabs(B[10])))) return;   // (an orthographic camera has no eye: no table)
#pragma unroll
    for (int j = 0; j < 3; j++) X.E[j] = B[8 + j] / B[11];
    X.why = 4;
    if (!(g.vpW > 0.0f && g.vpH > 0.0f) || !(fabs((double)g.depthRange) > 0.0)) return;
    X.why = 5;
    // the viewport's corners and its centre, one pixel beyond the image on every side (the sample offsets are below half a pixel)
    const double sxs[5] = {-1.0, (double)g.width, -1.0, (double)g.width, 0.5 * g.width}, sys[5] = {-1.0, -1.0, (double)g.height, (double)g.height, 0.5 * g.height};
    const double Zs[2] = {(0.0 - (double)g.minDepth) / (double)g.depthRange, (1.0 - (double)g.minDepth) / (double)g.depthRange};
    double Xm = 0.0, Ym = 0.0, aMin[2] = {1e300, 1e300}, pMax[2] = {0.0, 0.0}, vMax[2][4] = {{0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0}}, lMin = 1e300, dN = 0.0, oAx[3] = {0.0, 0.0, 0.0};
    double pws[5][2][3];
    int aSign = 0;
#pragma unroll
    for (int c = 0; c < 5; c++) {
        const double Xc = ((sxs[c] - X.vpX) / X.vpW) * 2.0 - 1.0, Yc = -(((sys[c] - X.vpY) / X.vpH) * 2.0 - 1.0);
        Xm = fmax(Xm, fabs(Xc)); Ym = fmax(Ym, fabs(Yc));
        double (&pw)[2][3] = pws[c], pb[3];
#pragma unroll
        for (int z = 0; z < 2; z++) {
            const double a = Xc * G[3] + Yc * G[7] + Zs[z] * G[11] + G[15];
            const int sg = a > 0.0 ? 1 : (a < 0.0 ? -1 : 0);
            if (sg == 0 || (aSign != 0 && sg != aSign)) return;   // (a is affine in X and Y: one sign at the corners is one sign over the viewport)
            aSign = sg;
            aMin[z] = fmin(aMin[z], fabs(a));
#pragma unroll
            for (int j = 0; j < 4; j++) vMax[z][j] = fmax(vMax[z][j], fabs(Xc * G[j] + Yc * G[4 + j] + Zs[z] * G[8 + j] + G[12 + j]));   // (affine in X and Y: largest at a corner)
            if (!scr_point(G, Xc, Yc, Zs[z], pw[z])) return;
            pMax[z] = fmax(pMax[z], sqrt(pw[z][0] * pw[z][0] + pw[z][1] * pw[z][1] + pw[z][2] * pw[z][2]));
        }
#pragma unroll
        for (int j = 0; j < 3; j++) oAx[j] = fmax(oAx[j], fabs(pw[0][j]));   // (the near points are convex combinations of the corners' up to the projective weights: the corners bound them)
        if (!scr_point(B, Xc, Yc, Zs[0], pb)) return;
        const double ex = pb[0] - X.E[0], ey = pb[1] - X.E[1], ez = pb[2] - X.E[2];
        dN = fmax(dN, sqrt(ex * ex + ey * ey + ez * ez));
    }
    // unproject in binary32, per component ((X m0 + Y m4) + Z m8) + m12: X and Y carry 4 u each, a product one rounding (none when Z is 0 or 1), a sum one rounding
    // of its own magnitude -- none when one side is an exact zero (a perspective matrix: a = Z m11 + m15 has ONE rounding although its terms cancel to 1 / far) --,
    // the last sum one rounding of the component itself; then the division by a: 1 / a and three products
    double eP[2];
#pragma unroll
    for (int z = 0; z < 2; z++) {
        double eC[4];
        const bool zExact = Zs[z] == 0.0 || Zs[z] == 1.0;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const double tx = Xm * fabs(G[j]), ty = Ym * fabs(G[4 + j]), tz = fabs(Zs[z]) * fabs(G[8 + j]);
            double e = (u * tx + 4.0 * u * fabs(G[j])) + (u * ty + 4.0 * u * fabs(G[4 + j])) + (zExact ? 0.0 : 5.0 * u * tz);
            if (tx > 0.0 && ty > 0.0) e += u * (tx + ty);
            if (tx + ty > 0.0 && tz > 0.0) e += u * (tx + ty + tz);
            e += u * vMax[z][j];
            eC[j] = 1.01 * e;
        }
        const double eNum = sqrt(eC[0] * eC[0] + eC[1] * eC[1] + eC[2] * eC[2]);
        eP[z] = 1.1 * (eNum + pMax[z] * eC[3]) / aMin[z] + 4.0 * u * pMax[z];
    }
    {   // |far - near| of a sample position is at least the far point's distance from the near points' plane; the far points fill a planar convex quad, on which that
        // distance is affine: smallest at a corner
        const double *n0 = pws[0][0], *n1 = pws[1][0], *n2 = pws[2][0];
        const double a1[3] = {n1[0] - n0[0], n1[1] - n0[1], n1[2] - n0[2]}, a2[3] = {n2[0] - n0[0], n2[1] - n0[1], n2[2] - n0[2]};
        const double nn[3] = {a1[1] * a2[2] - a1[2] * a2[1], a1[2] * a2[0] - a1[0] * a2[2], a1[0] * a2[1] - a1[1] * a2[0]};
        const double nl = sqrt(nn[0] * nn[0] + nn[1] * nn[1] + nn[2] * nn[2]);
        int sg = 0;
#pragma unroll
        for (int c = 0; c < 5 && nl > 0.0; c++) {
            const double *f = pws[c][1];
            const double d = (nn[0] * (f[0] - n0[0]) + nn[1] * (f[1] - n0[1]) + nn[2] * (f[2] - n0[2])) / nl;
            const int sd = d > 0.0 ? 1 : (d < 0.0 ? -1 : 0);
            if (sd == 0 || (sg != 0 && sd != sg)) { lMin = 0.0; break; }
            sg = sd;
            lMin = fmin(lMin, 0.999 * fabs(d));
        }
        if (!(nl > 0.0) || lMin > 1e299) lMin = 0.0;
    }
    X.why = 6;
    if (!(lMin > 0.0)) return;
    const double epsTW = 1.1 * (eP[0] + eP[1]) / lMin + 8.0 * u;   // normalize(far - near): the world direction
    // the body transform: ((x m0 + y m4) + z m8) + m12 per component, error <= 3.1 u of the terms' magnitudes; o + d first (one rounding of a number below oMax + 1)
    // (|M|_2 <= sqrt(|M|_1 |M|_inf) for the 3 x 3 part and for its inverse)
    double eV2 = 0.0, oN2 = 0.0;
#pragma unroll
    for (int j = 0; j < 3; j++) {
        const double cj = 3.1 * u * ((oAx[0] + eP[0] + 1.0) * fabs(IW[j]) + (oAx[1] + eP[0] + 1.0) * fabs(IW[4 + j]) + (oAx[2] + eP[0] + 1.0) * fabs(IW[8 + j]) + fabs(IW[12 + j]));
        eV2 += cj * cj;
        oN2 += (oAx[j] + eP[0] + 1.0) * (oAx[j] + eP[0] + 1.0);
    }
    const double eV = sqrt(eV2), oM = sqrt(oN2);
    const double c00 = IW[5] * IW[10] - IW[6] * IW[9], c01 = IW[6] * IW[8] - IW[4] * IW[10], c02 = IW[4] * IW[9] - IW[5] * IW[8];
    const double det = IW[0] * c00 + IW[1] * c01 + IW[2] * c02;
    X.why = 7;
    if (!(fabs(det) > 1e-300)) return;
    const double inv3[9] = {c00 / det, (IW[2] * IW[9] - IW[1] * IW[10]) / det, (IW[1] * IW[6] - IW[2] * IW[5]) / det,
                            c01 / det, (IW[0] * IW[10] - IW[2] * IW[8]) / det, (IW[2] * IW[4] - IW[0] * IW[6]) / det,
                            c02 / det, (IW[1] * IW[8] - IW[0] * IW[9]) / det, (IW[0] * IW[5] - IW[1] * IW[4]) / det};
    double n1 = 0.0, nInf = 0.0, i1 = 0.0, iInf = 0.0;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        n1 = fmax(n1, fabs(IW[k]) + fabs(IW[4 + k]) + fabs(IW[8 + k])); nInf = fmax(nInf, fabs(IW[4 * k]) + fabs(IW[4 * k + 1]) + fabs(IW[4 * k + 2]));
        i1 = fmax(i1, fabs(inv3[k]) + fabs(inv3[3 + k]) + fabs(inv3[6 + k])); iInf = fmax(iInf, fabs(inv3[3 * k]) + fabs(inv3[3 * k + 1]) + fabs(inv3[3 * k + 2]));
    }
    const double op = sqrt(n1 * nInf), lb = 1.0 / sqrt(i1 * iInf);   // |v x IW3| <= op |v|, >= lb |v|
    X.epsO = op * eP[0] + eV;
    X.epsT = 1.1 * (2.0 * eV + op * (epsTW + 1.01 * u * oM)) / lb + 8.0 * u;
    X.dN = dN + X.epsO;
    const double all = X.dN + X.epsO + X.epsT + fabs(X.E[0]) + fabs(X.E[1]) + fabs(X.E[2]);
    X.why = 8;
    if (!(all < 1e30) || !(X.epsT < 1e-2)) return;   // (NaNs fail both)
    X.why = 9;
    if (g.width > SCR_MAX_EXTENT || g.height > SCR_MAX_EXTENT) return;
    X.fx = 1.000001 * sqrt(X.F[0] * X.F[0] + X.F[4] * X.F[4] + X.F[8] * X.F[8]);
    X.fy = 1.000001 * sqrt(X.F[1] * X.F[1] + X.F[5] * X.F[5] + X.F[9] * X.F[9]);
    X.fw = 1.000001 * sqrt(X.F[3] * X.F[3] + X.F[7] * X.F[7] + X.F[11] * X.F[11]);
    if (!(X.fx + X.fy + X.fw < 1e30)) return;
    X.ok = 1; X.why = 0;
}

// The entry of one reference: its refT record's v1, E1, E2 -- the binary32 numbers RE:54-58 works on.
// Two parts.  delta(t), how far from the triangle the exact ray of an accepting sample position can pass, is a bound with a per cent of room: it is evaluated in
// binary32 (a few dozen roundings of positive terms; the two differences are taken with their errors on the safe side).  The projection is evaluated in double,
// except the reciprocal of w (binary32: 6e-8 of a coordinate of at most a few thousand pixels; `pad` below covers it).
XRT_HD ScrEntry screen_entry(const ScreenXf &X, const float *v1, const float *E1, const float *E2) {
    const ScrEntry none = {SCR_NO_CULL, SCR_NO_CULL};
    if (!X.ok) return none;
    const float u = 5.9604645e-8f;
    const float N[3] = {E1[1] * E2[2] - E1[2] * E2[1], E1[2] * E2[0] - E1[0] * E2[2], E1[0] * E2[1] - E1[1] * E2[0]};
    const float nn = sqrt_rn((N[0] * N[0] + N[1] * N[1]) + N[2] * N[2]);
    const float l1 = sqrt_rn((E1[0] * E1[0] + E1[1] * E1[1]) + E1[2] * E1[2]), l2 = sqrt_rn((E2[0] * E2[0] + E2[1] * E2[1]) + E2[2] * E2[2]);
    const float eMax = fmaxf(l1, l2), eMin = fminf(l1, l2);
    if (!(eMin >= 1e-9f && eMax <= 1e12f) || !(nn > 1e-6f * (l1 * l2))) return none;   // degenerate, or outside the magnitudes the error terms assume
    const float A = 1.0001f * (l1 * l2) / nn;
    const float Ef[3] = {(float)X.E[0], (float)X.E[1], (float)X.E[2]};
    float T[3][3], R2 = 0.0f;   // eye -> vertex k
    for (int k = 0; k < 3; k++) {
        for (int j = 0; j < 3; j++) T[k][j] = (v1[j] + (k == 1 ? E1[j] : (k == 2 ? E2[j] : 0.0f))) - Ef[j];
        R2 = fmaxf(R2, (T[k][0] * T[k][0] + T[k][1] * T[k][1]) + T[k][2] * T[k][2]);
    }
    const float eyeAbs = (fabsf(Ef[0]) + fabsf(Ef[1])) + fabsf(Ef[2]);
    const float R = 1.0001f * sqrt_rn(R2) + 4.0f * u * (eyeAbs + eMax);   // (the roundings of the differences above)
    const float dNf = 1.0001f * (float)X.dN;
    const float h = fabsf((N[0] * T[0][0] + N[1] * T[0][1]) + N[2] * T[0][2]) / nn;
    const float hMin = 0.9999f * h - dNf - 16.0f * u * (R + eyeAbs), tMax = R + dNf;   // the origin's distance from the triangle's plane, from its farthest vertex
    if (!(hMin > 0.0f)) return none;
    // (a) an accepting ray is not edge-on: cos >= min(1/2, cosLB), from the forward errors of row2, row3 and det alone
    const float cosLB = (0.429f * hMin * nn / eMax - 1.001f * u * (10.5f * eMax * tMax + 8.8f * eMax * eMax)) / (1.001f * (eMax * tMax + 1.01f * nn));
    const float c0 = fminf(0.5f, cosLB);
    if (!(c0 > 0.0f) || !(17.4f * u * A / c0 <= 0.5f)) return none;
    const float rhoC = 126.0f * u * (A / c0) * (tMax + eMax);
    // ... and with that margin: the ray meets the plane within rhoC of the triangle, so cos >= hMin / (tMax + rhoC)
    const float c1 = fmaxf(c0, 0.9999f * hMin / (tMax + rhoC + 2.0f * u * eMax));
    const float rho = 126.0f * u * (A / c1) * (tMax + eMax);
    // (c) the exact ray of the sample position passes as close to the triangle as the binary32 one, up to the origin's and the direction's error
    const float deltaF = 1.02f * (rho + 2.0f * u * eMax + (float)X.epsO + (tMax + rho) * (float)X.epsT);
    if (!(deltaF < 1e30f)) return none;
    const double delta = deltaF;
    // (b) the vertices on the screen, and how far a point within delta of the triangle can land from them: with s = x / w,
    // |s(q + e) - s(q)| <= delta (|Fx| + |s(q)| |Fw|) / (w(q) - delta |Fw|) for q in the triangle (all w > 0: s(q) lies between the vertices' s, w(q) above their least)
    double sxMin = 1e300, sxMax = -1e300, syMin = 1e300, syMax = -1e300, wMin = 1e300, padF = 0.0;
    for (int k = 0; k < 3; k++) {
        double p[3], v[4];
        for (int j = 0; j < 3; j++) p[j] = (double)v1[j] + (k == 1 ? (double)E1[j] : (k == 2 ? (double)E2[j] : 0.0));
        for (int j = 0; j < 4; j++) v[j] = p[0] * X.F[j] + p[1] * X.F[4 + j] + p[2] * X.F[8 + j] + X.F[12 + j];
        const double scale = fabs(v[0]) + fabs(v[1]) + fabs(v[2]) + fabs(v[3]);
        if (!(v[3] > 1e-3 * scale) || !(scale < 1e30)) return none;   // a vertex not clearly in front of the eye
        const double rw = (double)(1.0f / (float)v[3]);
        const double nx = v[0] * rw, ny = v[1] * rw;
        sxMin = fmin(sxMin, nx); sxMax = fmax(sxMax, nx); syMin = fmin(syMin, ny); syMax = fmax(syMax, ny); wMin = fmin(wMin, v[3]);
        // p x F is off by at most resid x scale per component (F = B^-1 (1 + R)): the quotients by (scale / w)(1 + |s|) resid
        padF = fmax(padF, 1.01 * (X.resid + 1e-15) * (scale * rw) * (1.0 + fmax(fabs(nx), fabs(ny))));
    }
    const double wLow = wMin - delta * X.fw;
    if (!(wLow > 0.5 * wMin)) return none;   // the grown triangle comes too near the eye's plane
    const double ax = fmax(fabs(sxMin), fabs(sxMax)), ay = fmax(fabs(syMin), fabs(syMax));
    if (!(ax < 64.0 && ay < 64.0)) return none;   // (far off the screen: the binary32 reciprocal above would cost more than `pad`)
    const double rl = 1.0001 * (double)(1.0f / (float)wLow);
    const double px = delta * (X.fx + ax * X.fw) * rl + padF, py = delta * (X.fy + ay * X.fw) * rl + padF;   // in NDC
    const double pad = 1e-9 * (X.vpW + X.vpH) + 0.0078125 + 1.3e-7 * (1.0 + fmax(ax, ay)) * fmax(X.vpW, X.vpH);   // this evaluation's own rounding, the binary32 reciprocals
    const double x0 = (sxMin - px + 1.0) * 0.5 * X.vpW + X.vpX, x1 = (sxMax + px + 1.0) * 0.5 * X.vpW + X.vpX;
    const double y0 = (1.0 - (syMax + py)) * 0.5 * X.vpH + X.vpY, y1 = (1.0 - (syMin - py)) * 0.5 * X.vpH + X.vpY;
    const double q[4] = {floor((x0 - pad) * SCR_UNITS) + SCR_BIAS, ceil((x1 + pad) * SCR_UNITS) + SCR_BIAS, floor((y0 - pad) * SCR_UNITS) + SCR_BIAS,
                         ceil((y1 + pad) * SCR_UNITS) + SCR_BIAS};
    unsigned f[4];
    for (int i = 0; i < 4; i++) {
        if (!(q[i] == q[i])) return none;
        f[i] = (unsigned)(q[i] < 0.0 ? 0.0 : (q[i] > (double)SCR_MAX ? (double)SCR_MAX : q[i]));
    }
    return ScrEntry{f[0] | (f[1] << 16), f[2] | (f[3] << 16)};
}

// The screen rectangle of a packet: the aligned block of `side` x `side` pixels at (x, y) with sample offsets of at most `off` sixteenths of a pixel.
XRT_HD ScrEntry screen_packet_rect(int x, int y, int side, int off) {
    const unsigned x0 = (unsigned)(SCR_UNITS * x - off + SCR_BIAS), x1 = (unsigned)(SCR_UNITS * (x + side - 1) + off + SCR_BIAS);
    const unsigned y0 = (unsigned)(SCR_UNITS * y - off + SCR_BIAS), y1 = (unsigned)(SCR_UNITS * (y + side - 1) + off + SCR_BIAS);
    return ScrEntry{x0 | (x1 << 16), y0 | (y1 << 16)};
}
// Can a ray of the packet be accepted by the entry's triangle?
XRT_HD bool screen_overlap(unsigned ex, unsigned ey, unsigned rx, unsigned ry) {
    const bool hit = ((ex & 0xffffu) <= (rx >> 16)) & ((ex >> 16) >= (rx & 0xffffu)) & ((ey & 0xffffu) <= (ry >> 16)) & ((ey >> 16) >= (ry & 0xffffu));
    return hit | (ex == SCR_NO_CULL);
}

}  // namespace xrt
