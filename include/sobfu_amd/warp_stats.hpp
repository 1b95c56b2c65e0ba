// Diagnostics of the deformation psi (no reference counterpart; kernel and rules: sobfu_amd/csrc/warp_stats_kernels.hip,
// sobfu_amd/csrc/sobfu_warp_stats.hpp): det J, folds, displacement and the residual of psi o psi^-1 in one pass, decoded
// from the C ABI's 64-word result block.  Part of sobfu.hpp, which includes it after DeviceArray and sobfuSafeCall: not a header to include
// on its own.  The Python twin is sobfu_amd.ops.warp_stats / WarpStats (the same decoding, operation by operation, and the same line).
#pragma once

namespace sobfu_amd {

struct WarpStats {
    int dims[3] = {0, 0, 0};
    bool has_inverse = false;
    unsigned long long words[SOBFU_WS_WORDS] = {};  // the raw result block
    // det J and the displacement over the voxels of the det mask; lengths in the units of the voxel size
    long long n_det = 0, n_fold = 0, n_det_nonfinite = 0, n_disp = 0, n_disp_nonfinite = 0;
    std::vector<float> edges;
    std::vector<long long> det_below;  // per edge: the voxels with det < edge
    double fold_fraction = 0, det_mean = 0, disp_mean = 0, res_mean = 0;  // NaN for an empty group
    float det_min = 0, det_max = 0, disp_max = 0, res_max = 0;            // NaN for an empty group
    int det_min_at[3] = {-1, -1, -1}, det_max_at[3] = {-1, -1, -1}, disp_max_at[3] = {-1, -1, -1}, res_max_at[3] = {-1, -1, -1};
    // the residual |psi(psi^-1(x)) - x| over the voxels of the residual mask
    long long n_res = 0, n_res_above = 0, n_res_outside = 0, n_res_nonfinite = 0;
};

namespace warp_stats_detail {
// (HI 2^24 + LO) 2^-44 / n in doubles, operation by operation (ops._ws_mean); NaN for an empty group
inline double mean(const unsigned long long* w, int at, long long n) {
    if (n == 0) return std::nan("");
    return ((double) (long long) w[at] * 16777216.0 + (double) (long long) w[at + 1]) / 17592186044416.0 / (double) n;
}
inline float key(unsigned long long k, bool maximum, const int dims[3], int at[3]) {
    at[0] = at[1] = at[2] = -1;
    if (k == ~0ULL) return std::nanf("");
    uint32_t o = (uint32_t) (k >> 32);
    const unsigned long long index = k & 0xffffffffULL;
    if (maximum) o = ~o;
    const uint32_t b = (o & 0x80000000u) ? (o ^ 0x80000000u) : ~o;
    float v;
    std::memcpy(&v, &b, 4);
    at[0] = (int) (index % (unsigned long long) dims[0]);
    at[1] = (int) ((index / (unsigned long long) dims[0]) % (unsigned long long) dims[1]);
    at[2] = (int) (index / ((unsigned long long) dims[0] * (unsigned long long) dims[1]));
    return v;
}
inline std::string g9(double v) {
    if (v != v) return "nan";
    char buf[64];
    std::snprintf(buf, sizeof buf, "%.9g", v);
    return buf;
}
}  // namespace warp_stats_detail

inline WarpStats decode_warp_stats(const unsigned long long* words, const int dims[3], const std::vector<float>& edges, bool has_inverse) {
    namespace d = warp_stats_detail;
    WarpStats s;
    std::memcpy(s.words, words, sizeof s.words);
    for (int i = 0; i < 3; ++i) s.dims[i] = dims[i];
    s.has_inverse = has_inverse, s.edges = edges;
    const unsigned long long* w = s.words;
    s.n_det = (long long) w[SOBFU_WS_N_DET], s.n_fold = (long long) w[SOBFU_WS_N_FOLD], s.n_det_nonfinite = (long long) w[SOBFU_WS_N_DET_NONFINITE];
    s.n_disp = (long long) w[SOBFU_WS_N_DISP], s.n_disp_nonfinite = (long long) w[SOBFU_WS_N_DISP_NONFINITE];
    s.n_res = (long long) w[SOBFU_WS_N_RES], s.n_res_above = (long long) w[SOBFU_WS_N_RES_ABOVE], s.n_res_outside = (long long) w[SOBFU_WS_N_RES_OUTSIDE];
    s.n_res_nonfinite = (long long) w[SOBFU_WS_N_RES_NONFINITE];
    for (size_t k = 0; k < edges.size(); ++k) s.det_below.push_back((long long) w[SOBFU_WS_DET_BELOW + k]);
    s.fold_fraction = s.n_det ? (double) s.n_fold / (double) s.n_det : std::nan("");
    s.det_mean = d::mean(w, SOBFU_WS_DET_SUM_HI, s.n_det), s.disp_mean = d::mean(w, SOBFU_WS_DISP_SUM_HI, s.n_disp), s.res_mean = d::mean(w, SOBFU_WS_RES_SUM_HI, s.n_res);
    s.det_min = d::key(w[SOBFU_WS_DET_MIN_KEY], false, dims, s.det_min_at), s.det_max = d::key(w[SOBFU_WS_DET_MAX_KEY], true, dims, s.det_max_at);
    s.disp_max = d::key(w[SOBFU_WS_DISP_MAX_KEY], true, dims, s.disp_max_at), s.res_max = d::key(w[SOBFU_WS_RES_MAX_KEY], true, dims, s.res_max_at);
    return s;
}

// One pass over psi (and psi_inv, mask, mask_inv when not null: device arrays of dims[0] x dims[1] x dims[2] float4 / float2 cells) ->
// WarpStats.  edges: up to 16 finite ascending det thresholds.  det / res (optional): the per-voxel volumes, downloaded.  Synchronises.
inline WarpStats warp_stats(const float* d_psi, const float* d_psi_inv, const float* d_mask, const float* d_mask_inv, const int dims[3], const float voxel_size[3],
                            float band, const std::vector<float>& edges, float res_tol, std::vector<float>* det = nullptr, std::vector<float>* res = nullptr) {
    const size_t n = (size_t) dims[0] * (size_t) dims[1] * (size_t) dims[2];
    kfusion::cuda::DeviceArray<unsigned long long> d_words(SOBFU_WS_WORDS);
    kfusion::cuda::DeviceArray<float> d_det, d_res;
    if (det) d_det.create(n);
    if (res && d_psi_inv) d_res.create(n);
    sobfuSafeCall(sobfu_hip_warp_stats(d_psi, d_psi_inv, d_mask, d_mask_inv, dims[0], dims[1], dims[2], voxel_size, band, edges.empty() ? nullptr : edges.data(),
                                       (int) edges.size(), res_tol, d_words.ptr(), det ? d_det.ptr() : nullptr, res && d_psi_inv ? d_res.ptr() : nullptr, nullptr));
    std::vector<unsigned long long> words;
    d_words.download(words);
    if (det) d_det.download(*det);
    if (res) {
        res->clear();
        if (d_psi_inv) d_res.download(*res);
    }
    return decode_warp_stats(words.data(), dims, edges, d_psi_inv != nullptr);
}

// "warp <n>: voxels=... det min=... @x,y,z max=... mean=... folds=... (...%) disp max=... mean=... inv res max=... @x,y,z mean=... above=... outside=..."
// (floats as %.9g: they round-trip); the inverse part only with psi_inv.  ops.WarpStats.line writes the same
inline std::string format_warp_stats(const WarpStats& s, int frame) {
    using warp_stats_detail::g9;
    std::string o = "warp " + std::to_string(frame) + ": voxels=" + std::to_string(s.n_det) + " det min=" + g9(s.det_min) + " @" + std::to_string(s.det_min_at[0]) + "," +
                    std::to_string(s.det_min_at[1]) + "," + std::to_string(s.det_min_at[2]) + " max=" + g9(s.det_max) + " mean=" + g9(s.det_mean) +
                    " folds=" + std::to_string(s.n_fold) + " (" + g9(100.0 * s.fold_fraction) + "%) disp max=" + g9(s.disp_max) + " mean=" + g9(s.disp_mean);
    if (s.has_inverse)
        o += " inv res max=" + g9(s.res_max) + " @" + std::to_string(s.res_max_at[0]) + "," + std::to_string(s.res_max_at[1]) + "," + std::to_string(s.res_max_at[2]) +
             " mean=" + g9(s.res_mean) + " above=" + std::to_string(s.n_res_above) + " outside=" + std::to_string(s.n_res_outside);
    return o;
}

}  // namespace sobfu_amd
