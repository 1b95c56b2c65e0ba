// Camera trajectories on the host (no reference counterpart; the C++ twin of sobfu_amd/trajectory.py): the TUM-format files
// apps/sobfu_headless --poses writes and --render-trajectory reads, and the two standard errors of an estimated trajectory against the
// true one (Sturm et al., "A benchmark for the evaluation of RGB-D SLAM systems", IROS 2012), in double precision.  Needs nothing but the
// standard library: a header to include on its own.  A pose is camera -> frame 0's camera, as SobFusion::getPoses.
#pragma once

#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

namespace sobfu_amd {

struct TrajectoryPose {
    int frame = 0;
    double t[3] = {0, 0, 0};
    double q[4] = {0, 0, 0, 1};  // x, y, z, w
};
typedef std::vector<TrajectoryPose> Trajectory;

// R (row-major) of a pose's quaternion, normalised first
inline void trajectory_rotation(const TrajectoryPose& p, double R[9]) {
    const double n = std::sqrt(p.q[0] * p.q[0] + p.q[1] * p.q[1] + p.q[2] * p.q[2] + p.q[3] * p.q[3]);
    const double x = p.q[0] / n, y = p.q[1] / n, z = p.q[2] / n, w = p.q[3] / n;
    R[0] = 1 - 2 * (y * y + z * z), R[1] = 2 * (x * y - z * w), R[2] = 2 * (x * z + y * w);
    R[3] = 2 * (x * y + z * w), R[4] = 1 - 2 * (x * x + z * z), R[5] = 2 * (y * z - x * w);
    R[6] = 2 * (x * z - y * w), R[7] = 2 * (y * z + x * w), R[8] = 1 - 2 * (x * x + y * y);
}

// (R row-major, t) -> a pose: q = (x, y, z, w) by Shepperd's branch on the largest diagonal term
template <class Real>
inline TrajectoryPose trajectory_pose(int frame, const Real R[9], const Real t[3]) {
    TrajectoryPose p;
    p.frame = frame;
    for (int i = 0; i < 3; ++i) p.t[i] = (double) t[i];
    double* q = p.q;
    const double tr = (double) R[0] + R[4] + R[8];
    if (tr > 0) {
        const double s = std::sqrt(tr + 1.0) * 2;
        q[3] = 0.25 * s, q[0] = (R[7] - R[5]) / s, q[1] = (R[2] - R[6]) / s, q[2] = (R[3] - R[1]) / s;
    } else if (R[0] > R[4] && R[0] > R[8]) {
        const double s = std::sqrt(1.0 + R[0] - R[4] - R[8]) * 2;
        q[3] = (R[7] - R[5]) / s, q[0] = 0.25 * s, q[1] = (R[1] + R[3]) / s, q[2] = (R[2] + R[6]) / s;
    } else if (R[4] > R[8]) {
        const double s = std::sqrt(1.0 + R[4] - R[0] - R[8]) * 2;
        q[3] = (R[2] - R[6]) / s, q[0] = (R[1] + R[3]) / s, q[1] = 0.25 * s, q[2] = (R[5] + R[7]) / s;
    } else {
        const double s = std::sqrt(1.0 + R[8] - R[0] - R[4]) * 2;
        q[3] = (R[3] - R[1]) / s, q[0] = (R[2] + R[6]) / s, q[1] = (R[5] + R[7]) / s, q[2] = 0.25 * s;
    }
    return p;
}

// one line per pose, "frame tx ty tz qx qy qz qw", the numbers at %.9g (which keeps every float)
inline bool write_tum(const std::string& path, const Trajectory& poses) {
    FILE* f = std::fopen(path.c_str(), "w");
    if (!f) return false;
    for (const TrajectoryPose& p : poses)
        std::fprintf(f, "%d %.9g %.9g %.9g %.9g %.9g %.9g %.9g\n", p.frame, p.t[0], p.t[1], p.t[2], p.q[0], p.q[1], p.q[2], p.q[3]);
    return std::fclose(f) == 0;
}

// Empty lines and lines that start with # are skipped; false + *why for any other line that is not eight numbers
inline bool read_tum(const std::string& path, Trajectory& poses, std::string* why = nullptr) {
    poses.clear();
    FILE* f = std::fopen(path.c_str(), "r");
    if (!f) {
        if (why) *why = "cannot open " + path;
        return false;
    }
    char line[1024];
    for (int ln = 1; std::fgets(line, sizeof line, f); ++ln) {
        const char* s = line;
        while (*s == ' ' || *s == '\t' || *s == '\r' || *s == '\n') ++s;
        if (*s == '\0' || *s == '#') continue;
        TrajectoryPose p;
        double frame = 0;
        char rest = 0;
        if (std::sscanf(s, "%lf %lf %lf %lf %lf %lf %lf %lf %c", &frame, &p.t[0], &p.t[1], &p.t[2], &p.q[0], &p.q[1], &p.q[2], &p.q[3], &rest) != 8) {
            if (why) *why = path + ":" + std::to_string(ln) + ": expected 'frame tx ty tz qx qy qz qw'";
            std::fclose(f);
            return false;
        }
        p.frame = (int) frame;
        poses.push_back(p);
    }
    std::fclose(f);
    return true;
}

namespace trajectory_detail {
// the eigenvector of the largest eigenvalue of a symmetric 4 x 4 matrix: cyclic Jacobi rotations
inline void top_eigenvector(double A[4][4], double v[4]) {
    double V[4][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1}};
    for (int sweep = 0; sweep < 64; ++sweep) {
        double off = 0, diag = 0;
        for (int i = 0; i < 4; ++i)
            for (int j = 0; j < 4; ++j) (i == j ? diag : off) += A[i][j] * A[i][j];
        if (off <= 1e-32 * diag || off == 0) break;
        for (int p = 0; p < 3; ++p)
            for (int q = p + 1; q < 4; ++q) {
                if (A[p][q] == 0) continue;
                const double theta = (A[q][q] - A[p][p]) / (2 * A[p][q]);
                const double t = (theta >= 0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1)), c = 1 / std::sqrt(t * t + 1), s = t * c;
                for (int k = 0; k < 4; ++k) {
                    const double akp = A[k][p], akq = A[k][q];
                    A[k][p] = c * akp - s * akq, A[k][q] = s * akp + c * akq;
                }
                for (int k = 0; k < 4; ++k) {
                    const double apk = A[p][k], aqk = A[q][k];
                    A[p][k] = c * apk - s * aqk, A[q][k] = s * apk + c * aqk;
                }
                for (int k = 0; k < 4; ++k) {
                    const double vkp = V[k][p], vkq = V[k][q];
                    V[k][p] = c * vkp - s * vkq, V[k][q] = s * vkp + c * vkq;
                }
            }
    }
    int best = 0;
    for (int i = 1; i < 4; ++i)
        if (A[i][i] > A[best][best]) best = i;
    for (int k = 0; k < 4; ++k) v[k] = V[k][best];
}
// pose_a^-1 pose_b: R = R_a^T R_b, t = R_a^T (t_b - t_a), every sum of products in a fixed order
inline void relative(const TrajectoryPose& a, const TrajectoryPose& b, double R[9], double t[3]) {
    double Ra[9], Rb[9];
    trajectory_rotation(a, Ra), trajectory_rotation(b, Rb);
    const double d[3] = {b.t[0] - a.t[0], b.t[1] - a.t[1], b.t[2] - a.t[2]};
    for (int i = 0; i < 3; ++i) {
        t[i] = (Ra[i] * d[0] + Ra[3 + i] * d[1]) + Ra[6 + i] * d[2];
        for (int j = 0; j < 3; ++j) R[3 * i + j] = (Ra[i] * Rb[j] + Ra[3 + i] * Rb[3 + j]) + Ra[6 + i] * Rb[6 + j];
    }
}
}  // namespace trajectory_detail

// The rigid transform (R row-major, t), no scale, that takes the positions of `est` closest to those of `gt` in the least-squares sense:
// Horn's closed form (JOSA A 4(4), 1987).  false: the trajectories differ in length or are empty
inline bool align_trajectory(const Trajectory& est, const Trajectory& gt, double R[9], double t[3]) {
    const size_t n = est.size();
    if (n == 0 || gt.size() != n) return false;
    double ca[3] = {0, 0, 0}, cb[3] = {0, 0, 0}, S[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
    for (size_t k = 0; k < n; ++k)
        for (int i = 0; i < 3; ++i) ca[i] += est[k].t[i] / (double) n, cb[i] += gt[k].t[i] / (double) n;
    for (size_t k = 0; k < n; ++k)
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) S[i][j] += (est[k].t[i] - ca[i]) * (gt[k].t[j] - cb[j]);
    double N[4][4] = {{S[0][0] + S[1][1] + S[2][2], S[1][2] - S[2][1], S[2][0] - S[0][2], S[0][1] - S[1][0]},
                      {S[1][2] - S[2][1], S[0][0] - S[1][1] - S[2][2], S[0][1] + S[1][0], S[2][0] + S[0][2]},
                      {S[2][0] - S[0][2], S[0][1] + S[1][0], S[1][1] - S[0][0] - S[2][2], S[1][2] + S[2][1]},
                      {S[0][1] - S[1][0], S[2][0] + S[0][2], S[1][2] + S[2][1], S[2][2] - S[0][0] - S[1][1]}};
    double q[4];  // w, x, y, z
    trajectory_detail::top_eigenvector(N, q);
    TrajectoryPose p;
    p.q[0] = q[1], p.q[1] = q[2], p.q[2] = q[3], p.q[3] = q[0];
    trajectory_rotation(p, R);
    for (int i = 0; i < 3; ++i) t[i] = cb[i] - ((R[3 * i] * ca[0] + R[3 * i + 1] * ca[1]) + R[3 * i + 2] * ca[2]);
    return true;
}

// absolute trajectory error: the root mean square of the distances between the positions of `gt` and those of `est` after
// align_trajectory; NaN where that fails
inline double ate(const Trajectory& est, const Trajectory& gt) {
    double R[9], t[3], sum = 0;
    if (!align_trajectory(est, gt, R, t)) return NAN;
    for (size_t k = 0; k < est.size(); ++k)
        for (int i = 0; i < 3; ++i) {
            const double d = ((R[3 * i] * est[k].t[0] + R[3 * i + 1] * est[k].t[1]) + R[3 * i + 2] * est[k].t[2]) + t[i] - gt[k].t[i];
            sum += d * d;
        }
    return std::sqrt(sum / (double) est.size());
}

// relative pose error over steps of `delta` frames: with A_i = est_i^-1 est_(i + delta) and B_i likewise of gt, E_i = B_i^-1 A_i ->
// *trans, the root mean square of |trans(E_i)| (metres), and *rot, that of the rotation angle of E_i (radians): atan2 of the length of the
// skew part of rot(E_i) and (trace - 1) / 2.  A trajectory against itself gives exactly (0, 0).  false: lengths differ, or too few poses
inline bool rpe(const Trajectory& est, const Trajectory& gt, double* trans, double* rot, int delta = 1) {
    const size_t n = est.size();
    if (gt.size() != n || delta < 1 || n <= (size_t) delta) return false;
    double st = 0, sr = 0;
    for (size_t k = 0; k + delta < n; ++k) {
        double Ra[9], ta[3], Rb[9], tb[3], E[9];
        trajectory_detail::relative(est[k], est[k + delta], Ra, ta);
        trajectory_detail::relative(gt[k], gt[k + delta], Rb, tb);
        const double d[3] = {ta[0] - tb[0], ta[1] - tb[1], ta[2] - tb[2]};
        for (int i = 0; i < 3; ++i) {
            const double c = (Rb[i] * d[0] + Rb[3 + i] * d[1]) + Rb[6 + i] * d[2];
            st += c * c;
            for (int j = 0; j < 3; ++j) E[3 * i + j] = (Rb[i] * Ra[j] + Rb[3 + i] * Ra[3 + j]) + Rb[6 + i] * Ra[6 + j];
        }
        const double sx = E[7] - E[5], sy = E[2] - E[6], sz = E[3] - E[1];
        const double angle = std::atan2(0.5 * std::sqrt((sx * sx + sy * sy) + sz * sz), 0.5 * (((E[0] + E[4]) + E[8]) - 1.0));
        sr += angle * angle;
    }
    const double m = (double) (n - (size_t) delta);
    *trans = std::sqrt(st / m), *rot = std::sqrt(sr / m);
    return true;
}

}  // namespace sobfu_amd
