// local_map_bench.cpp -- times the four local-map calls (plslam_local_map_form / _candidates / _gather / _cull) host to host
// against what a caller has to do without them for the same results: plain C++ loops over the same CSR image on the host plus the
// upload of the two candidate masks the _dev map<->keyframe drivers read.  The baseline is written here, independently of the
// library.  Both paths run in ONE process, alternating, after a warm-up; medians and minima per call; one JSON line.
//   usage: local_map_bench <n_pt> <n_ls> <n_kf> <window> <rounds>
//   build: g++ -O2 -std=c++17 -D__HIP_PLATFORM_AMD__ tools/local_map_bench.cpp -Iinclude -I/opt/rocm/include
//          -Lplslam_amd/lib -lplslam_hip -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,$PWD/plslam_amd/lib -Wl,-rpath,/opt/rocm/lib
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "plslam_hip.h"

struct Kind {
    int dl, dv;
    std::vector<uint8_t> valid, inlier;
    std::vector<double> X, val;
    std::vector<int32_t> optr, okf, fptr, fidx;
};
static uint64_t g_s = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() { g_s = g_s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(g_s >> 33); }

static Kind make_kind(int n, int n_kf, int dl, int dv)
{
    Kind k{dl, dv, {}, {}, {}, {}, {0}, {}, {}, {}};
    std::vector<std::vector<int32_t>> feats(n_kf);
    for (int i = 0; i < n; ++i) {
        k.valid.push_back(rnd() % 20 != 0);
        k.inlier.push_back(rnd() % 10 != 0);
        for (int a = 0; a < dl; ++a) k.X.push_back((double)(rnd() % 4000) / 100.0 - 20.0);
        const int no = 1 + (int)(rnd() % 5), first = (int)(rnd() % n_kf);
        for (int o = 0; o < no; ++o) {
            const int kf = std::min(n_kf - 1, first + o * (int)(1 + rnd() % 3));      // ascending keyframes
            k.okf.push_back(kf);
            for (int a = 0; a < dv; ++a) k.val.push_back((double)(rnd() % 70000) / 100.0);
            feats[kf].push_back(i);
            if (rnd() % 4 == 0) feats[kf].push_back(-1);
        }
        k.optr.push_back((int32_t)k.okf.size());
    }
    k.fptr.push_back(0);
    for (auto& f : feats) { k.fidx.insert(k.fidx.end(), f.begin(), f.end()); k.fptr.push_back((int32_t)k.fidx.size()); }
    return k;
}

struct HostOut {                                             // what the baseline produces (sizes only are reported)
    std::vector<uint8_t> kf_local, local[2], cand[2], removed[2];
    std::vector<int32_t> kf_list, list[2], obs6[2];
    std::vector<double> X_aux, val[2];
};

template <class T> static T* dev(const std::vector<T>& v)
{
    void* d = nullptr;
    if (hipMalloc(&d, v.size() * sizeof(T) + 8) != hipSuccess) { fprintf(stderr, "hipMalloc failed\n"); exit(1); }
    if (!v.empty() && hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) exit(1);
    return static_cast<T*>(d);
}
static double now_us() { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
static void stat(std::vector<double> v, double& med, double& mn) { std::sort(v.begin(), v.end()); med = v[v.size() / 2]; mn = v[0]; }
#define CK(x) do { int rc_ = (x); if (rc_ != PLSLAM_OK) { fprintf(stderr, "%s: %s; %s\n", #x, plslam_strerror(rc_), plslam_last_error()); return 1; } } while (0)

int main(int argc, char** argv)
{
    const int n_pt = argc > 1 ? atoi(argv[1]) : 10000, n_ls = argc > 2 ? atoi(argv[2]) : 2500, n_kf = argc > 3 ? atoi(argv[3]) : 200,
              window = argc > 4 ? atoi(argv[4]) : 29, rounds = argc > 5 ? atoi(argv[5]) : 30;
    Kind K[2] = {make_kind(n_pt, n_kf, 3, 2), make_kind(n_ls, n_kf, 6, 3)};
    std::vector<uint8_t> kf_valid(n_kf, 1);
    std::vector<double> x_kf(6 * (size_t)n_kf, 0.1);
    std::vector<int32_t> row(n_kf, 0);
    const int anchor = n_kf - 1, min_cov = 75, kf2 = n_kf - 1, max_kf_idx = n_kf + 5, min_lm_obs = 3;

    plslam_ctx* ctx = nullptr;
    CK(plslam_ctx_create(0, &ctx));
    plslam_map_index map{};
    map.n_map_kf = n_kf; map.kf_valid = dev(kf_valid); map.x_kf_w = dev(x_kf);
    plslam_map_landmarks* ML[2] = {&map.points, &map.lines};
    for (int k = 0; k < 2; ++k) {
        plslam_map_landmarks& L = *ML[k];
        L.n = (int32_t)K[k].valid.size(); L.n_obs = (int32_t)K[k].okf.size(); L.n_feat = (int32_t)K[k].fidx.size();
        L.valid = dev(K[k].valid); L.inlier = dev(K[k].inlier); L.X = dev(K[k].X); L.obs_ptr = dev(K[k].optr); L.obs_kf = dev(K[k].okf);
        L.obs_val = dev(K[k].val); L.feat_ptr = dev(K[k].fptr); L.feat_idx = dev(K[k].fidx);
    }
    uint8_t* d_mask[2] = {dev(std::vector<uint8_t>(n_pt + 8)), dev(std::vector<uint8_t>(n_ls + 8))};
    plslam_local_map* lm = nullptr;
    CK(plslam_local_map_create(ctx, &lm));
    plslam_local_map_counts c{};
    std::vector<double> t_dev[4], t_host[4];
    HostOut h;
    for (int r = 0; r < rounds + 3; ++r) {
        // ---- the device calls -------------------------------------------------------------------------------------------
        double t0 = now_us();
        CK(plslam_local_map_form(lm, &map, anchor, row.data(), min_cov, window, &c));
        double t1 = now_us();
        CK(plslam_local_map_candidates(lm, &map, kf2));
        double t2 = now_us();
        CK(plslam_local_map_gather(lm, &map, &c));
        double t3 = now_us();
        CK(plslam_local_map_cull(lm, &map, max_kf_idx, min_lm_obs, &c));
        double t4 = now_us();
        for (int k = 0; k < 2; ++k) {                        // (outside the windows: the culled image is put back)
            (void)hipMemcpy(ML[k]->valid, K[k].valid.data(), K[k].valid.size(), hipMemcpyHostToDevice);
            (void)hipMemcpy(ML[k]->feat_idx, K[k].fidx.data(), K[k].fidx.size() * 4, hipMemcpyHostToDevice);
        }
        // ---- the host loops a caller writes without them, + the mask upload ---------------------------------------------
        Kind W[2] = {K[0], K[1]};                            // (outside the windows: a working copy the cull may change)
        double u0 = now_us();
        h.kf_local.assign(n_kf, 0);
        for (int k = 0; k < 2; ++k) h.local[k].assign(W[k].valid.size(), 0);
        for (int i = 0; i < n_kf; ++i) {
            if (!kf_valid[i] || !(i == anchor || (i < n_kf - 1 && (row[i] >= min_cov || n_kf - 1 - i <= window)))) continue;
            h.kf_local[i] = 1;
            for (int k = 0; k < 2; ++k)
                for (int32_t f = W[k].fptr[i]; f < W[k].fptr[i + 1]; ++f) {
                    const int32_t idx = W[k].fidx[f];
                    if (idx >= 0 && W[k].valid[idx]) h.local[k][idx] = 1;
                }
        }
        double u1 = now_us();
        for (int k = 0; k < 2; ++k) {
            const size_t n = W[k].valid.size();
            h.cand[k].assign(n, 0);
            for (size_t i = 0; i < n; ++i)
                h.cand[k][i] = W[k].valid[i] && h.local[k][i] && W[k].optr[i + 1] > W[k].optr[i] && W[k].okf[W[k].optr[i + 1] - 1] != kf2;
            if (n) (void)hipMemcpy(d_mask[k], h.cand[k].data(), n, hipMemcpyHostToDevice);
        }
        double u2 = now_us();
        h.kf_list.clear(); h.X_aux.clear();
        std::vector<int32_t> inv(n_kf, -1);
        for (int i = 1; i < n_kf; ++i)
            if (kf_valid[i] && h.kf_local[i]) {
                inv[i] = (int32_t)h.kf_list.size();
                h.kf_list.push_back(i);
                h.X_aux.insert(h.X_aux.end(), x_kf.begin() + 6 * i, x_kf.begin() + 6 * i + 6);
            }
        for (int k = 0; k < 2; ++k) {
            h.list[k].clear(); h.obs6[k].clear(); h.val[k].clear();
            for (size_t i = 0; i < W[k].valid.size(); ++i) {
                if (!W[k].valid[i] || !h.local[k][i]) continue;
                const int32_t loc = (int32_t)h.list[k].size();
                h.X_aux.insert(h.X_aux.end(), W[k].X.begin() + W[k].dl * i, W[k].X.begin() + W[k].dl * (i + 1));
                for (int32_t o = W[k].optr[i]; o < W[k].optr[i + 1]; ++o) {
                    const int32_t kf = W[k].okf[o];
                    const int32_t r6[6] = {(int32_t)i, loc, o - W[k].optr[i], kf, inv[kf], 1};
                    h.obs6[k].insert(h.obs6[k].end(), r6, r6 + 6);
                    h.val[k].insert(h.val[k].end(), W[k].val.begin() + (size_t)W[k].dv * o, W[k].val.begin() + (size_t)W[k].dv * (o + 1));
                }
                h.list[k].push_back((int32_t)i);
            }
        }
        double u3 = now_us();
        for (int k = 0; k < 2; ++k) {
            h.removed[k].assign(W[k].valid.size(), 0);
            for (size_t i = 0; i < W[k].valid.size(); ++i) {
                const int32_t b = W[k].optr[i], e = W[k].optr[i + 1];
                if (!W[k].valid[i] || h.local[k][i] || e == b || !(max_kf_idx - W[k].okf[b] > 10)) continue;
                if (W[k].inlier[i] && !(e - b < min_lm_obs)) continue;
                const int32_t kf = W[k].okf[b];
                for (int32_t f = W[k].fptr[kf]; f < W[k].fptr[kf + 1]; ++f)
                    if (W[k].fidx[f] == (int32_t)i) { W[k].fidx[f] = -1; break; }
                W[k].valid[i] = 0;
                h.removed[k][i] = 1;
            }
        }
        double u4 = now_us();
        if (r < 3) continue;                                 // warm-up
        const double d[4] = {t1 - t0, t2 - t1, t3 - t2, t4 - t3}, u[4] = {u1 - u0, u2 - u1, u3 - u2, u4 - u3};
        for (int q = 0; q < 4; ++q) { t_dev[q].push_back(d[q]); t_host[q].push_back(u[q]); }
    }
    // the two paths computed the same lists (lengths and removals; the tests compare contents)
    size_t rem = 0;
    for (int k = 0; k < 2; ++k) for (uint8_t r : h.removed[k]) rem += r;
    const bool same = c.nkf == (int32_t)h.kf_list.size() && c.npt == (int32_t)h.list[0].size() && c.nls == (int32_t)h.list[1].size() &&
                      c.n_pt_obs == (int32_t)(h.obs6[0].size() / 6) && c.n_ls_obs == (int32_t)(h.obs6[1].size() / 6) &&
                      (size_t)(c.n_pt_removed + c.n_ls_removed) == rem;
    const char* names[4] = {"form", "candidates", "gather", "cull"};
    printf("{\"n_pt\": %d, \"n_ls\": %d, \"n_kf\": %d, \"nkf_local\": %d, \"npt_local\": %d, \"n_pt_obs\": %d, \"removed\": %zu, \"same_counts\": %s, \"rounds\": %d",
           n_pt, n_ls, n_kf, c.nkf, c.npt, c.n_pt_obs, rem, same ? "true" : "false", rounds);
    double sd = 0, sh = 0;
    for (int q = 0; q < 4; ++q) {
        double md, mnd, mh, mnh;
        stat(t_dev[q], md, mnd); stat(t_host[q], mh, mnh);
        sd += md; sh += mh;
        printf(", \"%s_us\": {\"device_median\": %.1f, \"device_min\": %.1f, \"host_median\": %.1f, \"host_min\": %.1f}", names[q], md, mnd, mh, mnh);
    }
    printf(", \"sum_of_medians_us\": {\"device\": %.1f, \"host\": %.1f}}\n", sd, sh);
    plslam_local_map_destroy(lm);
    plslam_ctx_destroy(ctx);
    return same ? 0 : 3;
}
