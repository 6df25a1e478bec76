// The float64 eigen-solve of a symmetric 3x3 covariance and the bound on its distance from LAPACK's decomposition of the same matrix:
// ONE definition for lrg_preprocess (eig_mode 1 / 2) and lrg_baseline_eig.
#pragma once

// |Jacobi - LAPACK| in units of the largest singular value: both solvers are backward stable with a constant of a few eps, 256 eps
// is an order of magnitude above either (learn_region_grow_amd.preprocess_gpu.EXACT_SLACK is the same number)
#define PREP_EIG_SLACK (256.0 * 2.220446049250313e-16)
// Eigen-decomposition of a symmetric 3x3 matrix, cyclic Jacobi in float64.  w: eigenvalues, V[k][:]: eigenvector k.
__device__ void prep_jacobi3(const double *c, double *w, double (*V)[3]) {
    double a[3][3] = {{c[0], c[1], c[2]}, {c[1], c[4], c[5]}, {c[2], c[5], c[8]}};
    double v[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};             // columns = eigenvectors
    for (int sweep = 0; sweep < 30; ++sweep) {
        const double off = fabs(a[0][1]) + fabs(a[0][2]) + fabs(a[1][2]);
        const double diag = fabs(a[0][0]) + fabs(a[1][1]) + fabs(a[2][2]);
        if (off == 0.0 || off <= 1e-300 || off < 1e-22 * diag) break;
        for (int p = 0; p < 2; ++p)
            for (int q = p + 1; q < 3; ++q) {
                const double apq = a[p][q];
                if (apq == 0.0) continue;
                const double theta = (a[q][q] - a[p][p]) / (2.0 * apq);
                const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double cs = 1.0 / sqrt(t * t + 1.0), sn = t * cs;
                const int r = 3 - p - q;
                const double app = a[p][p], aqq = a[q][q], arp = a[r][p], arq = a[r][q];
                a[p][p] = app - t * apq;
                a[q][q] = aqq + t * apq;
                a[p][q] = a[q][p] = 0.0;
                a[r][p] = a[p][r] = cs * arp - sn * arq;
                a[r][q] = a[q][r] = sn * arp + cs * arq;
                for (int k = 0; k < 3; ++k) {
                    const double vkp = v[k][p], vkq = v[k][q];
                    v[k][p] = cs * vkp - sn * vkq;
                    v[k][q] = sn * vkp + cs * vkq;
                }
            }
    }
    for (int k = 0; k < 3; ++k) { w[k] = a[k][k]; V[k][0] = v[0][k]; V[k][1] = v[1][k]; V[k][2] = v[2][k]; }
}

// singular values of a symmetric matrix = |eigenvalues|: which is the largest (i0), the middle (i1) and the smallest (i2), with the
// tie rules of numpy.linalg.svd's descending order as prep_eig_point has always applied them
__device__ __forceinline__ void prep_eig_order(const double *s, int *i0_out, int *i1_out, int *i2_out) {
    int i0 = 0, i2 = 0;
    if (s[1] > s[i0]) i0 = 1;
    if (s[2] > s[i0]) i0 = 2;
    if (s[1] < s[i2]) i2 = 1;
    if (s[2] <= s[i2]) i2 = 2;
    if (i0 == i2) { i0 = 0; i2 = 2; }                                                               // all equal
    *i0_out = i0; *i1_out = 3 - i0 - i2; *i2_out = i2;
}
