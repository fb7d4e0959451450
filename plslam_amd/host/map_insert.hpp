// map_insert.hpp -- header-only client of the map insertion on the device (plslam_map_insert_*, include/plslam_hip.h): MapImages
// keeps the CSR image of the map (plslam_map_index) on the device in TWO copies with room to grow and runs the insertion loops of
// MapHandler::matchKF2KFPoints / Lines (src/mapHandler.cpp:280-360, :428-527) and matchMap2KFPoints / Lines (:601-629, :716-749)
// from one into the other, so that the image never travels: index() is what plslam_local_map_* take next.  The caller keeps
// full_graph (row_delta) and map_*_kf_idx (the events); desc_list / dir_list / pts_list follow on the device with map_lists.hpp's
// MapLists::carry.  No PL-SLAM type here; the HIP runtime is used for the images' device memory only.
#pragma once

#include <hip/hip_runtime_api.h>

#include <stdexcept>
#include <string>
#include <vector>

#include "plslam_hip.h"

namespace PLSLAM {
namespace map_insert {

struct HostKind {                                                       // one landmark kind of the image, as plslam_map_index lays it out
    std::vector<uint8_t> valid, inlier;
    std::vector<double> X, obs_val;
    std::vector<int32_t> obs_ptr, obs_kf, feat_ptr, feat_idx;
};
struct HostImage {
    std::vector<uint8_t> kf_valid;
    std::vector<double> x_kf_w;
    HostKind points, lines;
};
struct KindMatches {                                                    // one kind of one keyframe; an empty table: no entry
    std::vector<int32_t> table;                                         // matches_12 (kf2kf) or map_to_kf (map2kf)
    std::vector<double> P1, obs1, P2, obs2;                             // P / sP eP and pl / le of kf1's and kf2's features
};
struct Event {
    int lm, i1, i2;
    bool is_new;
    double dir_first[3], dir[3];                                        // the new landmark's first observation; the kf2 observation
};
struct Inserted {
    std::vector<Event> pt_events, ls_events;
    std::vector<int32_t> row_delta;                                     // += into full_graph[kf2][.] and full_graph[.][kf2]
    plslam_map_insert_counts counts;
};

inline void check(int rc, const char* where)
{
    if (rc != PLSLAM_OK) throw std::runtime_error(std::string("[map_insert] ") + where + ": " + plslam_strerror(rc) + "; " + plslam_last_error());
}
inline void hip_check(hipError_t e, const char* where)
{
    if (e != hipSuccess) throw std::runtime_error(std::string("[map_insert] ") + where + ": " + hipGetErrorString(e));
}

class MapImages {
public:
    explicit MapImages(plslam_ctx* ctx) { check(plslam_map_insert_create(ctx, &mi_), "create"); }
    ~MapImages()
    {
        plslam_map_insert_destroy(mi_);
        for (Image& im : img_) release(im);
    }
    MapImages(const MapImages&) = delete;
    MapImages& operator=(const MapImages&) = delete;

    // the image the calls read next (device pointers)
    const plslam_map_index& index() const { return img_[cur_].d.map; }
    // the image the last insert / pingpong READ, and the handle whose records describe that call (map_lists.hpp)
    const plslam_map_index& previous() const { return img_[1 - cur_].d.map; }
    plslam_map_insert* handle() const { return mi_; }

    // uploads a host image (every keyframe slot, kf2 included, is in it)
    void upload(const HostImage& h)
    {
        Image& im = img_[cur_];
        const int32_t nk = (int32_t)h.kf_valid.size();
        reserve(im, nk, sizes(h.points), sizes(h.lines));
        put(im.d.map.kf_valid, h.kf_valid); put(im.d.map.x_kf_w, h.x_kf_w);
        im.d.map.n_map_kf = nk;
        put_kind(im.d.map.points, h.points);
        put_kind(im.d.map.lines, h.lines);
    }
    void download(HostImage& h) const
    {
        const plslam_map_index& m = index();
        get(h.kf_valid, m.kf_valid, (size_t)m.n_map_kf); get(h.x_kf_w, m.x_kf_w, 6 * (size_t)m.n_map_kf);
        get_kind(h.points, m.points, m.n_map_kf, 3, 2);
        get_kind(h.lines, m.lines, m.n_map_kf, 6, 3);
    }
    // matchKF2KFPoints + matchKF2KFLines: the loops behind the matchers (:280-360, :428-527)
    Inserted insertKF2KF(int kf1_idx, int kf2_idx, const double T_kf1_w[16], const double T_kf2_w[16], const KindMatches& pts,
                         const KindMatches& lns)
    {
        return run(false, kf1_idx, kf2_idx, T_kf1_w, T_kf2_w, pts, lns);
    }
    // matchMap2KFPoints + matchMap2KFLines: the loops behind the gates (:601-629, :716-749); table = map_to_kf
    Inserted insertMap2KF(int kf2_idx, const double T_kf2_w[16], const KindMatches& pts, const KindMatches& lns)
    {
        return run(true, -1, kf2_idx, nullptr, T_kf2_w, pts, lns);
    }
    // another out-of-place call of the library over the pair (host/lc_fuse.hpp): the other image is given room for the stated
    // landmarks and observations per kind, f(current index, destination) runs the call, and the images swap when it returns
    template <class F> void pingpong(int32_t pt_n, int32_t pt_n_obs, int32_t ls_n, int32_t ls_n_obs, F&& f)
    {
        const plslam_map_index& m = img_[cur_].d.map;
        Image& dst = img_[1 - cur_];
        reserve(dst, m.n_map_kf, Sizes{pt_n, pt_n_obs, m.points.n_feat}, Sizes{ls_n, ls_n_obs, m.lines.n_feat});
        f(m, dst.d);
        cur_ = 1 - cur_;
    }

private:
    struct Sizes { int32_t n, n_obs, n_feat; };
    struct Image { plslam_map_insert_dst d{}; int32_t kf_cap = 0, pt_feat_cap = 0, ls_feat_cap = 0; std::vector<void*> blocks; };
    static Sizes sizes(const HostKind& k) { return Sizes{(int32_t)k.valid.size(), (int32_t)k.obs_kf.size(), (int32_t)k.feat_idx.size()}; }
    static Sizes sizes(const plslam_map_landmarks& k) { return Sizes{k.n, k.n_obs, k.n_feat}; }
    static void release(Image& im)
    {
        for (void* p : im.blocks) (void)hipFree(p);
        im = Image{};
    }
    template <class T> static T* dev(Image& im, size_t n)
    {
        void* d = nullptr;
        hip_check(hipMalloc(&d, n * sizeof(T) + 8), "hipMalloc");
        im.blocks.push_back(d);
        return static_cast<T*>(d);
    }
    template <class T, class U> static void put(U* d, const std::vector<T>& v)
    {
        if (!v.empty()) hip_check(hipMemcpy((void*)d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice), "hipMemcpy");
    }
    template <class T, class U> static void get(std::vector<T>& v, const U* d, size_t n)
    {
        v.resize(n);
        if (n) hip_check(hipMemcpy(v.data(), (const void*)d, n * sizeof(T), hipMemcpyDeviceToHost), "hipMemcpy");
    }
    static void put_kind(plslam_map_landmarks& L, const HostKind& k)
    {
        L.n = (int32_t)k.valid.size(); L.n_obs = (int32_t)k.obs_kf.size(); L.n_feat = (int32_t)k.feat_idx.size();
        put(L.valid, k.valid); put(L.inlier, k.inlier); put(L.X, k.X); put(L.obs_ptr, k.obs_ptr); put(L.obs_kf, k.obs_kf);
        put(L.obs_val, k.obs_val); put(L.feat_ptr, k.feat_ptr); put(L.feat_idx, k.feat_idx);
    }
    static void get_kind(HostKind& k, const plslam_map_landmarks& L, int32_t nk, int dl, int dv)
    {
        get(k.valid, L.valid, (size_t)L.n); get(k.inlier, L.inlier, (size_t)L.n); get(k.X, L.X, (size_t)dl * L.n);
        get(k.obs_ptr, L.obs_ptr, (size_t)L.n + 1); get(k.obs_kf, L.obs_kf, (size_t)L.n_obs); get(k.obs_val, L.obs_val, (size_t)dv * L.n_obs);
        get(k.feat_ptr, L.feat_ptr, (size_t)nk + 1); get(k.feat_idx, L.feat_idx, (size_t)L.n_feat);
    }
    // an image with room for these sizes; it is rebuilt half as large again when it is too small (its content is NOT kept:
    // the caller writes all of it next)
    static void reserve(Image& im, int32_t nk, Sizes p, Sizes l)
    {
        if (nk <= im.kf_cap && p.n <= im.d.pt_cap && p.n_obs <= im.d.pt_obs_cap && l.n <= im.d.ls_cap && l.n_obs <= im.d.ls_obs_cap &&
            p.n_feat <= im.pt_feat_cap && l.n_feat <= im.ls_feat_cap)
            return;
        release(im);
        auto grow = [](int32_t n) { return n + n / 2 + 64; };
        im.kf_cap = grow(nk);
        im.d.pt_cap = grow(p.n); im.d.pt_obs_cap = grow(p.n_obs); im.d.ls_cap = grow(l.n); im.d.ls_obs_cap = grow(l.n_obs);
        im.pt_feat_cap = grow(p.n_feat); im.ls_feat_cap = grow(l.n_feat);
        im.d.map.kf_valid = dev<uint8_t>(im, im.kf_cap);
        im.d.map.x_kf_w = dev<double>(im, 6 * (size_t)im.kf_cap);
        auto kind = [&](plslam_map_landmarks& L, int32_t cap, int32_t ocap, int32_t fcap, int dl, int dv) {
            L.valid = dev<uint8_t>(im, cap); L.inlier = dev<uint8_t>(im, cap); L.X = dev<double>(im, (size_t)dl * cap);
            L.obs_ptr = dev<int32_t>(im, (size_t)cap + 1); L.obs_kf = dev<int32_t>(im, ocap); L.obs_val = dev<double>(im, (size_t)dv * ocap);
            L.feat_ptr = dev<int32_t>(im, (size_t)im.kf_cap + 1); L.feat_idx = dev<int32_t>(im, fcap);
        };
        kind(im.d.map.points, im.d.pt_cap, im.d.pt_obs_cap, im.pt_feat_cap, 3, 2);
        kind(im.d.map.lines, im.d.ls_cap, im.d.ls_obs_cap, im.ls_feat_cap, 6, 3);
    }
    static plslam_map_insert_kind kind_arg(const KindMatches& k)
    {
        plslam_map_insert_kind a{};
        a.table = k.table.empty() ? nullptr : k.table.data();
        a.n_table = (int32_t)k.table.size();
        a.P1 = k.P1.data(); a.obs1 = k.obs1.data(); a.P2 = k.P2.data(); a.obs2 = k.obs2.data();
        return a;
    }
    static int32_t matched(const KindMatches& k)
    {
        int32_t m = 0;
        for (int32_t v : k.table) m += v >= 0;
        return m;
    }
    Inserted run(bool map2kf, int kf1, int kf2, const double* T1, const double* T2, const KindMatches& pts, const KindMatches& lns)
    {
        const Image& src = img_[cur_];
        Image& dst = img_[1 - cur_];
        const plslam_map_index& m = src.d.map;
        Sizes p = sizes(m.points), l = sizes(m.lines);
        const int32_t mp = matched(pts), ml = matched(lns);
        p.n += map2kf ? 0 : mp; p.n_obs += (map2kf ? 1 : 2) * mp;      // the bound the tables give
        l.n += map2kf ? 0 : ml; l.n_obs += (map2kf ? 1 : 2) * ml;
        reserve(dst, m.n_map_kf, p, l);
        plslam_map_insert_kind ap = kind_arg(pts), al = kind_arg(lns);
        ap.n_prev = map2kf ? 0 : (int32_t)(pts.obs1.size() / 2); ap.n_curr = (int32_t)(pts.obs2.size() / 2);
        al.n_prev = map2kf ? 0 : (int32_t)(lns.obs1.size() / 3); al.n_curr = (int32_t)(lns.obs2.size() / 3);
        Inserted out;
        out.row_delta.assign((size_t)m.n_map_kf, 0);
        check(map2kf ? plslam_map_insert_map2kf(mi_, &m, &dst.d, kf2, T2, &ap, &al, out.row_delta.data(), &out.counts)
                     : plslam_map_insert_kf2kf(mi_, &m, &dst.d, kf1, kf2, T1, T2, &ap, &al, out.row_delta.data(), &out.counts),
              map2kf ? "map2kf" : "kf2kf");
        cur_ = 1 - cur_;
        std::vector<int32_t> pe(4 * (size_t)out.counts.points.n_events), le(4 * (size_t)out.counts.lines.n_events);
        std::vector<double> pd(6 * (size_t)out.counts.points.n_events), ld(6 * (size_t)out.counts.lines.n_events);
        plslam_map_insert_events h{};
        h.pt_ev = pe.data(); h.pt_dir = pd.data(); h.ls_ev = le.data(); h.ls_dir = ld.data();
        check(plslam_map_insert_download(mi_, &h), "download");
        auto events = [](const std::vector<int32_t>& e, const std::vector<double>& d, std::vector<Event>& o) {
            o.resize(e.size() / 4);
            for (size_t k = 0; k < o.size(); ++k) {
                o[k].lm = e[4 * k]; o[k].i1 = e[4 * k + 1]; o[k].i2 = e[4 * k + 2]; o[k].is_new = e[4 * k + 3] != 0;
                for (int a = 0; a < 3; ++a) { o[k].dir_first[a] = d[6 * k + a]; o[k].dir[a] = d[6 * k + 3 + a]; }
            }
        };
        events(pe, pd, out.pt_events);
        events(le, ld, out.ls_events);
        return out;
    }
    plslam_map_insert* mi_ = nullptr;
    Image img_[2];
    int cur_ = 0;
};

}  // namespace map_insert
}  // namespace PLSLAM
