// map_lists.hpp -- header-only client of the map's side lists on the device (plslam_map_lists_*, plslam_map_insert_carry,
// plslam_lc_fuse_carry; include/plslam_hip.h): MapLists keeps desc_list / dir_list / pts_list and the representative descriptor
// (MapPoint / MapLine::med_desc, src/mapFeatures.cpp:51-84) of every landmark on the device in TWO copies with room to grow,
// beside the pair of images map_insert.hpp's MapImages keeps, and carries them from one into the other behind every insert
// (MapImages::insertKF2KF / insertMap2KF) and every fusion (lc_fuse::Fuser::run): lists().points.med_desc is what
// plslam_map2kf_match_points_dev takes next as d_med_desc, lists().points.dir with the image's obs_ptr what
// plslam_lc_correct_map_dev takes as dirs / dir_ptr.  The carries only enqueue; download() and the next carry wait.
// No PL-SLAM type here; the HIP runtime is used for the lists' device memory only.
#pragma once

#include "lc_fuse.hpp"

namespace PLSLAM {
namespace map_lists {

using map_insert::check;
using map_insert::hip_check;
using map_insert::MapImages;

struct HostKind {                                                       // one kind, rows in the image's observation / landmark order
    std::vector<uint8_t> desc;                                          // n_obs x 32
    std::vector<double> dir, pts;                                       // n_obs x 3; n_obs x 4 (lines)
    std::vector<int32_t> med_idx;                                       // n
    std::vector<uint8_t> med_desc, refreshed;                           // n x 32; n
};
struct HostLists { HostKind points, lines; };
// the rows of one kind an insert or a fusion brings: a = keyframe 1's (n_prev; kf2kf only) or per tuple kf_prev's, b = keyframe
// 2's (n_curr) or per tuple kf_curr's; pts (x 4: spl, epl) for lines
struct Rows {
    std::vector<uint8_t> desc_a, desc_b;
    std::vector<double> pts_a, pts_b;
};

class MapLists {
public:
    explicit MapLists(plslam_ctx* ctx) : ctx_(ctx) {}
    ~MapLists()
    {
        (void)hipDeviceSynchronize();
        drop_staged();
        for (Lists& l : l_) release(l);
    }
    MapLists(const MapLists&) = delete;
    MapLists& operator=(const MapLists&) = delete;

    // the lists that go with the image the calls read next (device pointers)
    const plslam_map_lists& lists() const { return l_[cur_].d; }

    // uploads the lists of `map` (desc / dir / pts; med_idx / med_desc too unless refresh: then they are computed on the device)
    void upload(const HostLists& h, const plslam_map_index& map, bool refresh)
    {
        Lists& l = l_[cur_];
        reserve(l, map.points.n, map.points.n_obs, map.lines.n, map.lines.n_obs);
        put_kind(l.d.points, h.points, !refresh);
        put_kind(l.d.lines, h.lines, !refresh);
        if (refresh) check(plslam_map_lists_refresh(ctx_, &map, &l.d), "map_lists_refresh");
    }
    void download(HostLists& h, const plslam_map_index& map) const
    {
        hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");
        get_kind(h.points, l_[cur_].d.points, map.points, false);
        get_kind(h.lines, l_[cur_].d.lines, map.lines, true);
    }
    // behind maps.insertKF2KF / insertMap2KF: the lists follow the image the insert wrote
    void carry(MapImages& maps, const Rows& pts, const Rows& lns)
    {
        const plslam_map_index& dst = maps.index();
        Lists& out = begin(dst);
        const plslam_map_insert_rows rp{stage(pts.desc_a), stage(pts.desc_b), nullptr, nullptr};
        const plslam_map_insert_rows rl{stage(lns.desc_a), stage(lns.desc_b), stage(lns.pts_a), stage(lns.pts_b)};
        check(plslam_map_insert_carry(maps.handle(), &maps.previous(), &l_[cur_].d, &dst, &out.d, &rp, &rl), "map_insert_carry");
        cur_ = 1 - cur_;
    }
    // behind fuser.run(maps, ...): rows per tuple, gathered as lc_fuse::pack gathers P0 / P1
    void carry(lc_fuse::Fuser& fuser, MapImages& maps, const Rows& pts, const Rows& lns)
    {
        const plslam_map_index& dst = maps.index();
        Lists& out = begin(dst);
        const plslam_lc_fuse_rows rp{stage(pts.desc_a), stage(pts.desc_b), nullptr, nullptr};
        const plslam_lc_fuse_rows rl{stage(lns.desc_a), stage(lns.desc_b), stage(lns.pts_a), stage(lns.pts_b)};
        check(plslam_lc_fuse_carry(fuser.handle(), &maps.previous(), &l_[cur_].d, &dst, &out.d, &rp, &rl), "lc_fuse_carry");
        cur_ = 1 - cur_;
    }

private:
    struct Lists { plslam_map_lists d{}; int32_t cap[2] = {0, 0}, obs_cap[2] = {0, 0}; std::vector<void*> blocks; };
    static void release(Lists& l)
    {
        for (void* p : l.blocks) (void)hipFree(p);
        l = Lists{};
    }
    template <class T> static T* dev(std::vector<void*>& blocks, size_t n)
    {
        void* d = nullptr;
        hip_check(hipMalloc(&d, n * sizeof(T) + 16), "hipMalloc");     // (hipMalloc's blocks are 256-byte aligned: the calls want 16)
        blocks.push_back(d);
        return static_cast<T*>(d);
    }
    // the other copy with room for the image `dst`; what the last carry left in flight is waited for, its staged rows go
    Lists& begin(const plslam_map_index& dst)
    {
        hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");
        drop_staged();
        Lists& out = l_[1 - cur_];
        reserve(out, dst.points.n, dst.points.n_obs, dst.lines.n, dst.lines.n_obs);
        return out;
    }
    void drop_staged()
    {
        for (void* p : staged_) (void)hipFree(p);
        staged_.clear();
    }
    template <class T> const T* stage(const std::vector<T>& v)
    {
        if (v.empty()) return nullptr;
        T* d = dev<T>(staged_, v.size());
        hip_check(hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice), "hipMemcpy");
        return d;
    }
    // lists with room for these sizes; rebuilt half as large again when too small (the content is NOT kept: the caller writes
    // all of it next)
    static void reserve(Lists& l, int32_t pn, int32_t pobs, int32_t ln, int32_t lobs)
    {
        if (pn <= l.cap[0] && pobs <= l.obs_cap[0] && ln <= l.cap[1] && lobs <= l.obs_cap[1]) return;
        release(l);
        auto grow = [](int32_t n) { return n + n / 2 + 64; };
        l.cap[0] = grow(pn); l.obs_cap[0] = grow(pobs); l.cap[1] = grow(ln); l.obs_cap[1] = grow(lobs);
        auto kind = [&](plslam_map_lists_kind& K, int32_t cap, int32_t ocap, bool lines) {
            K.desc = dev<uint8_t>(l.blocks, 32 * (size_t)ocap); K.dir = dev<double>(l.blocks, 3 * (size_t)ocap);
            K.pts = lines ? dev<double>(l.blocks, 4 * (size_t)ocap) : nullptr;
            K.med_idx = dev<int32_t>(l.blocks, cap); K.med_desc = dev<uint8_t>(l.blocks, 32 * (size_t)cap); K.refreshed = dev<uint8_t>(l.blocks, cap);
        };
        kind(l.d.points, l.cap[0], l.obs_cap[0], false);
        kind(l.d.lines, l.cap[1], l.obs_cap[1], true);
    }
    template <class T> static void put(T* d, const std::vector<T>& v)
    {
        if (d && !v.empty()) hip_check(hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice), "hipMemcpy");
    }
    template <class T> static void get(std::vector<T>& v, const T* d, size_t n)
    {
        v.resize(d ? n : 0);
        if (d && n) hip_check(hipMemcpy(v.data(), d, n * sizeof(T), hipMemcpyDeviceToHost), "hipMemcpy");
    }
    static void put_kind(plslam_map_lists_kind& K, const HostKind& h, bool with_med)
    {
        put(K.desc, h.desc); put(K.dir, h.dir); put(K.pts, h.pts);
        if (with_med) { put(K.med_idx, h.med_idx); put(K.med_desc, h.med_desc); }
    }
    static void get_kind(HostKind& h, const plslam_map_lists_kind& K, const plslam_map_landmarks& m, bool lines)
    {
        get(h.desc, (const uint8_t*)K.desc, 32 * (size_t)m.n_obs); get(h.dir, (const double*)K.dir, 3 * (size_t)m.n_obs);
        get(h.pts, (const double*)(lines ? K.pts : nullptr), 4 * (size_t)m.n_obs);
        get(h.med_idx, (const int32_t*)K.med_idx, (size_t)m.n); get(h.med_desc, (const uint8_t*)K.med_desc, 32 * (size_t)m.n);
        get(h.refreshed, (const uint8_t*)K.refreshed, (size_t)m.n);
    }
    plslam_ctx* ctx_;
    Lists l_[2];
    std::vector<void*> staged_;
    int cur_ = 0;
};

}  // namespace map_lists
}  // namespace PLSLAM
