// rtmi_update.hip — host unit of the scene updates (include/rtmi_update.h): the entry points, the tables a
// handle builds on its first update and the ordering of an update among the calls on the handle.  No kernel here: the
// scatter and the refit are reached through rtmi_update_launch.hpp.  rtmu_refittable and rtmu_refit_desc are the host
// evaluation of rtmi_refit.hpp and touch no device.  On a handle that follows its lights (include/rtmi_relight.h; §44) an
// update that moves an emitter also enqueues the relight kernel, through rtmi_relight_launch.hpp.
#include "rtmi_host.hpp"

#include "rtmi_update.h"
#include "rtmi_relight.hpp"

#define UPD_TRY(expr) RTMI_HIP_TRY("rtmu_scene_update_prims: ", false, expr, #expr)
#define UPX_TRY(expr) RTMI_HIP_TRY("rtmu_scene_update_xforms: ", false, expr, #expr)

// what a transform record is to rtmu_scene_update_xforms: in no chain (a gate or inner-medium record, or unused), in an
// item's chain, in the chain of a primitive of a LIST item, in that of a primitive inside a BVH item, in a deferred group
enum { UP_XF_NONE = 0, UP_XF_ITEM = 1, UP_XF_PRIM = 2, UP_XF_IN_TREE = 3, UP_XF_GROUP = 4 };

extern "C" int rtmu_refittable(const rtmi_scene_desc *desc, uint8_t *mask) {
    std::string err;
    const int rc = refit_refittable(desc, mask, err);
    return rc ? fail(rc, "rtmu_refittable", err.c_str()) : RTMI_OK;
}

extern "C" int rtmu_refit_desc(const rtmi_scene_desc *desc, uint32_t first, uint32_t count, rtmi_item *items, rtmi_bvh_node *nodes,
                               rtmi_bvh4_node *alt_nodes, float *prim_gate) {
    std::string err;
    const int rc = refit_desc(desc, first, count, items, nodes, alt_nodes, prim_gate, err);
    return rc ? fail(rc, "rtmu_refit_desc", err.c_str()) : RTMI_OK;
}

// The handle does not keep its description (s->meta holds borrowed pointers): what the refit needs is read back from the
// device arrays once.  The children of the alternative trees come back pool-encoded and are decoded for the plan.
static int build_tables(rtmi_scene *s) {
    const rtmi_scene_desc &m = s->meta;
    if (s->busy_recorded) UPD_TRY(hipEventSynchronize(s->busy.e));
    std::vector<DevItem> ditems(m.n_items);
    std::vector<rtmi_bvh_node> nodes(m.n_nodes);
    std::vector<rtmi_bvh4_node> alt(s->dev.nodes4 ? m.n_alt_nodes : 0u);
    std::vector<rtmi_prim_meta> meta(m.n_prims);
    std::vector<rtmi_material> mats(m.n_materials);
    if (!ditems.empty()) UPD_TRY(hipMemcpy(ditems.data(), s->dev.items, ditems.size() * sizeof(DevItem), hipMemcpyDeviceToHost));
    if (!nodes.empty()) UPD_TRY(hipMemcpy(nodes.data(), s->dev.nodes, nodes.size() * sizeof(rtmi_bvh_node), hipMemcpyDeviceToHost));
    if (!alt.empty()) UPD_TRY(hipMemcpy(alt.data(), s->dev.nodes4, alt.size() * sizeof(rtmi_bvh4_node), hipMemcpyDeviceToHost));
    if (!meta.empty()) UPD_TRY(hipMemcpy(meta.data(), s->dev.meta, meta.size() * sizeof(rtmi_prim_meta), hipMemcpyDeviceToHost));
    if (!mats.empty()) UPD_TRY(hipMemcpy(mats.data(), s->dev.mats, mats.size() * sizeof(rtmi_material), hipMemcpyDeviceToHost));
    for (rtmi_bvh4_node &n : alt)
        for (int c = 0; c < 4; c++) {
            const uint32_t e = (uint32_t)n.child[c];
            if (e == 0xffffffffu) n.child[c] = RTMI_NO_CHILD;
            else if (e & (1u << 25)) n.child[c] = RTMI_LEAF((e >> 22) & 7u, e & 0x003fffffu);
        }
    std::vector<rtmi_item> items(m.n_items);
    std::vector<int32_t> medium_item(m.n_prims ? m.n_prims : 1u, -1);
    for (uint32_t i = 0; i < m.n_items; i++) {
        items[i] = ditems[i].it;
        if ((items[i].flags & RTMI_ITEMFLAG_DEV_MEDIUM_SPHERE) && items[i].first >= 0 && (uint32_t)items[i].first < m.n_prims)
            medium_item[(size_t)items[i].first] = (int32_t)i;
        items[i].flags &= ~RTMI_ITEMFLAG_DEV_MEDIUM_SPHERE;
    }
    rtmi_scene_desc d{};
    d.n_items = m.n_items; d.items = items.data();
    d.n_prims = m.n_prims; d.prim_meta = meta.data();
    d.n_nodes = m.n_nodes; d.nodes = nodes.data();
    d.n_alt_nodes = (uint32_t)alt.size(); d.alt_nodes = alt.data();
    RefitPlan plan;
    if (int rc = refit_plan_build(&d, plan)) return fail(rc, "rtmu_scene_update_prims", plan.err.c_str());

    std::vector<uint32_t> words;
    std::vector<RefitJob> jobs;
    const auto lists = [&](const std::vector<uint32_t> &order, const std::vector<uint32_t> &lvl, uint32_t &at, uint32_t &n_lvl) {
        at = (uint32_t)words.size();
        n_lvl = lvl.empty() ? 0u : (uint32_t)lvl.size() - 1u;
        const uint32_t base = at + (uint32_t)lvl.size();
        for (uint32_t o : lvl) words.push_back(base + o);
        words.insert(words.end(), order.begin(), order.end());
    };
    for (uint32_t i = 0; i < m.n_items; i++) {
        const RefitPlanItem &P = plan.items[i];
        if (!P.bvh || !P.refittable) continue;
        RefitJob J{};
        J.item = i; J.root = (uint32_t)items[i].first;
        J.prim_lo = P.prim_lo; J.prim_hi = P.prim_hi;
        lists(P.order, P.lvl, J.lvl, J.n_lvl);
        lists(P.alt_order, P.alt_lvl, J.alt_lvl, J.alt_n_lvl);
        jobs.push_back(J);
    }
    if (words.empty()) words.push_back(0u);
    UPD_TRY(s->up_words.alloc(words.size() * sizeof(uint32_t)));
    UPD_TRY(hipMemcpy(s->up_words.ptr, words.data(), words.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    UPD_TRY(s->up_jobs.alloc((jobs.empty() ? 1u : jobs.size()) * sizeof(RefitJob)));
    if (!jobs.empty()) UPD_TRY(hipMemcpy(s->up_jobs.ptr, jobs.data(), jobs.size() * sizeof(RefitJob), hipMemcpyHostToDevice));
    UPD_TRY(s->up_medium_item.alloc(medium_item.size() * sizeof(int32_t)));
    UPD_TRY(hipMemcpy(s->up_medium_item.ptr, medium_item.data(), medium_item.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    UPD_TRY(s->up_scratch.alloc((size_t)(m.n_nodes ? m.n_nodes : 1u) * 2 * sizeof(float4)));
    s->up_n_jobs = (uint32_t)jobs.size();
    s->up_type.assign(m.n_prims, 0);
    s->up_emits.assign(m.n_prims, 0);
    for (uint32_t p = 0; p < m.n_prims; p++) {
        s->up_type[p] = (uint8_t)meta[p].type;
        const int32_t mt = meta[p].material;
        s->up_emits[p] = mt >= 0 && (uint32_t)mt < m.n_materials && mats[(size_t)mt].kind == RTMI_MAT_DIFFUSE_LIGHT ? 1 : 0;
    }
    // the transform records: whose chain each lies in
    std::vector<rtmi_xform> xf(m.n_xforms);
    if (!xf.empty()) UPD_TRY(hipMemcpy(xf.data(), s->dev.xforms, xf.size() * sizeof(rtmi_xform), hipMemcpyDeviceToHost));
    s->up_xf_kind.assign(m.n_xforms, 0);
    s->up_xf_item.assign(m.n_xforms, -1);
    s->up_xf_slot.assign(m.n_xforms, 0);
    s->up_xf_state.assign(m.n_xforms, UP_XF_NONE);
    for (uint32_t k = 0; k < m.n_xforms; k++) s->up_xf_kind[k] = xf[k].kind;
    const auto grouped = [&](const rtmi_item &it) { return (it.flags & (RTMI_ITEMFLAG_SAVE_T0 | RTMI_ITEMFLAG_DEFERRED)) != 0u; };
    for (uint32_t i = 0; i < m.n_items; i++)
        for (int32_t k = 0; k < items[i].xform_count; k++) {
            const int64_t at = (int64_t)items[i].xform_first + k;
            if (at < 0 || at >= (int64_t)m.n_xforms) continue;
            s->up_xf_item[(size_t)at] = (int32_t)i;
            s->up_xf_slot[(size_t)at] = k;
            s->up_xf_state[(size_t)at] = grouped(items[i]) ? UP_XF_GROUP : UP_XF_ITEM;
        }
    for (uint32_t p = 0; p < m.n_prims; p++) {
        const uint32_t cnt = (meta[p].flags >> RTMI_PRIMFLAG_XF_COUNT_SHIFT) & RTMI_PRIM_XF_MAX, at = meta[p].flags >> RTMI_PRIMFLAG_XF_FIRST_SHIFT;
        const int32_t owner = plan.prim_item[p];
        for (uint32_t k = 0; k < cnt && at + k < m.n_xforms; k++)
            s->up_xf_state[at + k] = owner < 0 || grouped(items[(size_t)owner]) ? UP_XF_GROUP : items[(size_t)owner].kind == RTMI_ITEM_BVH ? UP_XF_IN_TREE : UP_XF_PRIM;
    }
    s->up_plan = std::move(plan);
    s->up_ready = true;
    return RTMI_OK;
}

// the checks of an update up to its first enqueue; the caller holds s->mu and has selected the device
static int admit(rtmi_scene *s, uint32_t first, uint32_t count) {
    if ((uint64_t)first + (uint64_t)count > s->meta.n_prims) return fail(RTMI_ERR_INVALID, "rtmu_scene_update_prims", "the range leaves the primitives");
    if (s->has_f64)
        return fail(RTMI_ERR_UNSUPPORTED, "rtmu_scene_update_prims", "the handle has f64 planes attached, which an update would leave stale");
    if (!s->up_ready)
        if (int rc = build_tables(s)) return rc;
    std::vector<uint8_t> touched;
    if (int rc = refit_touched(s->up_plan, first, count, touched)) return fail(rc, "rtmu_scene_update_prims", s->up_plan.err.c_str());
    return RTMI_OK;
}

// scatter and refit on `stream`, after the previous call on the handle; the handle's `busy` event follows them
static int enqueue(rtmi_scene *s, uint32_t first, uint32_t count, const float *d_a, const float *d_b, hipStream_t stream) {
    bool relight = false;
    for (uint32_t p = first; p < first + count; p++)
        if (s->up_emits[p]) { // the light table and the tree over it hold copies of this geometry
            if (s->rl_on && s->rl_ready && s->has_lights) { // following (rtmi_relight.h): they are recomputed behind the refit
                relight = true;
            } else {
                s->has_lights = false;
                s->has_light_tree = false;
            }
            break;
        }
    if (s->busy_recorded) UPD_TRY(hipStreamWaitEvent(stream, s->busy.e, 0));
    BusyMark busy{s, stream};
    UpdateScene U{};
    U.items = reinterpret_cast<char *>(const_cast<DevItem *>(s->dev.items));
    U.prim_a = const_cast<float4 *>(s->dev.prim_a); U.prim_b = const_cast<float4 *>(s->dev.prim_b);
    U.gate = const_cast<float4 *>(s->dev.gate);
    U.nodes = const_cast<float4 *>(s->dev.nodes); U.nodes4 = const_cast<float4 *>(s->dev.nodes4);
    U.leaf_rec = const_cast<float4 *>(s->dev.leaf_rec); U.shade_prim = const_cast<float4 *>(s->dev.shade_prim);
    U.words = s->up_words.ptr; U.jobs = s->up_jobs.ptr; U.medium_item = s->up_medium_item.ptr; U.scratch = s->up_scratch.ptr;
    U.n_jobs = s->up_n_jobs;
    UPD_TRY(rtmi_update_scatter_launch(stream, U, first, count, d_a, d_b));
    UPD_TRY(rtmi_update_refit_launch(stream, U, first, count));
    if (relight) {
        RelightScene R{};
        R.prim_a = s->dev.prim_a; R.prim_b = s->dev.prim_b;
        R.lights = reinterpret_cast<float *>(s->nee_lights.ptr);
        R.n = s->nee_n;
        R.weight = s->rl_weight.ptr; R.words = s->rl_words.ptr;
        R.aw = s->rl_scratch.ptr; R.box = s->rl_scratch.ptr + (s->nee_n ? s->nee_n : 1u);
        const bool tree = s->has_light_tree && s->rl_n_lvl > 0u; // the tables were built over this tree: attaching another turns following off
        R.nodes = tree ? reinterpret_cast<float *>(s->lt_nodes.ptr) : nullptr;
        R.n_lvl = tree ? s->rl_n_lvl : 0u;
        UPD_TRY(rtmi_relight_launch(stream, R));
    }
    return RTMI_OK;
}

extern "C" int rtmu_scene_update_prepare(rtmi_scene *s) {
    if (!s) return fail(RTMI_ERR_INVALID, "rtmu_scene_update_prepare", "scene is NULL");
    std::lock_guard<std::mutex> lock(s->mu);
    UPD_TRY(hipSetDevice(s->device));
    return s->up_ready ? RTMI_OK : build_tables(s);
}

extern "C" int rtmu_scene_update_prims_device(rtmi_scene *s, uint32_t first, uint32_t count, const void *d_a, const void *d_b, void *stream) {
    if (!s) return fail(RTMI_ERR_INVALID, "rtmu_scene_update_prims_device", "scene is NULL");
    std::lock_guard<std::mutex> lock(s->mu);
    UPD_TRY(hipSetDevice(s->device));
    if (count == 0 && first <= s->meta.n_prims) return RTMI_OK;
    if (!d_a || misaligned(d_a, 4) || misaligned(d_b, 4)) return fail(RTMI_ERR_INVALID, "rtmu_scene_update_prims_device", "d_a is NULL or a plane is not 4-byte aligned");
    if (int rc = admit(s, first, count)) return rc; // (after the caller's pointers: an invalid call does no device work)
    return enqueue(s, first, count, static_cast<const float *>(d_a), static_cast<const float *>(d_b), reinterpret_cast<hipStream_t>(stream));
}

extern "C" int rtmu_scene_update_prims(rtmi_scene *s, uint32_t first, uint32_t count, const float *a, const float *b) {
    const char *name = "rtmu_scene_update_prims";
    if (!s) return fail(RTMI_ERR_INVALID, name, "scene is NULL");
    std::lock_guard<std::mutex> lock(s->mu);
    UPD_TRY(hipSetDevice(s->device));
    if (count == 0 && first <= s->meta.n_prims) return RTMI_OK;
    if (!a) return fail(RTMI_ERR_INVALID, name, "a is NULL");
    if (int rc = admit(s, first, count)) return rc;
    for (uint32_t i = 0; i < count; i++) {
        const uint32_t p = first + i;
        const float *A = a + (size_t)i * 4, *B = b ? b + (size_t)i * 4 : nullptr;
        const int32_t owner = s->up_plan.prim_item[p];
        if (owner < 0 || !s->up_plan.items[(size_t)owner].bvh) continue; // a list primitive sits under no box: as at creation, any value
        // what the refit reads of a primitive inside a tree must be finite: plane A, and a cube's max.y, max.z in plane B
        for (int k = 0; k < 4; k++)
            if (!finite_f(A[k]) || (B && k < 2 && s->up_type[p] == RTMI_PRIM_CUBE && !finite_f(B[k])))
                return fail(RTMI_ERR_INVALID, name, "a plane of a primitive of a refittable item is not finite");
        if (s->up_type[p] == RTMI_PRIM_SPHERE && !(A[3] > 0.0f)) return fail(RTMI_ERR_INVALID, name, "a sphere of a refittable item needs a positive radius");
        if (s->up_type[p] == RTMI_PRIM_CUBE && (A[0] > A[3] || (B && (A[1] > B[0] || A[2] > B[1]))))
            return fail(RTMI_ERR_INVALID, name, "a cube of a refittable item is inverted (min > max)");
    }
    if (s->rl_on && s->rl_ready && s->has_lights) // following: a listed light must stay a light (rtmi_relight.h)
        for (uint32_t i = 0; i < count; i++) {
            const int32_t li = s->rl_prim_light[first + i];
            if (li < 0) continue;
            if (const char *why = relight_degenerate(s->rl_plane[(size_t)li], a + (size_t)i * 4, s->rl_weight_h[(size_t)li]))
                return fail(RTMI_ERR_INVALID, name, (std::string("the handle follows its lights and the new planes make ") + why).c_str());
        }
    if (int rc = begin_blocking(s)) return rc;
    const size_t plane = (size_t)count * 4;
    UPD_TRY(s->up_h_stage.grow(2 * plane * sizeof(float)));
    UPD_TRY(s->up_stage.grow(2 * plane * sizeof(float)));
    memcpy(s->up_h_stage.ptr, a, plane * sizeof(float));
    if (b) memcpy(s->up_h_stage.ptr + plane, b, plane * sizeof(float));
    UPD_TRY(hipMemcpyAsync(s->up_stage.ptr, s->up_h_stage.ptr, (b ? 2 : 1) * plane * sizeof(float), hipMemcpyHostToDevice, s->stream.s));
    if (int rc = enqueue(s, first, count, s->up_stage.ptr, b ? s->up_stage.ptr + plane : nullptr, s->stream.s)) return rc;
    UPD_TRY(hipStreamSynchronize(s->stream.s));
    return RTMI_OK;
}

extern "C" int rtmu_scene_update_xforms(rtmi_scene *s, uint32_t first, uint32_t count, const rtmi_xform *recs) {
    const char *name = "rtmu_scene_update_xforms";
    if (!s) return fail(RTMI_ERR_INVALID, name, "scene is NULL");
    std::lock_guard<std::mutex> lock(s->mu);
    UPX_TRY(hipSetDevice(s->device));
    if ((uint64_t)first + (uint64_t)count > s->meta.n_xforms) return fail(RTMI_ERR_INVALID, name, "the range leaves the transform records");
    if (count == 0) return RTMI_OK;
    if (!recs) return fail(RTMI_ERR_INVALID, name, "recs is NULL");
    if (s->has_f64) return fail(RTMI_ERR_UNSUPPORTED, name, "the handle has f64 planes attached, which an update would leave stale");
    if (!s->up_ready)
        if (int rc = build_tables(s)) return rc;
    for (uint32_t k = 0; k < count; k++) {
        const rtmi_xform &r = recs[k];
        if (r.kind != s->up_xf_kind[first + k] || r.kind < RTMI_XF_TRANSLATE || r.kind > RTMI_XF_ROTATE_Z)
            return fail(RTMI_ERR_INVALID, name, "a record must keep its kind, which must be TRANSLATE or ROTATE_*");
        if (!finite_f(r.x) || !finite_f(r.y) || !finite_f(r.z)) return fail(RTMI_ERR_INVALID, name, "a record is not finite");
        switch (s->up_xf_state[first + k]) {
        case UP_XF_ITEM: case UP_XF_PRIM: break;
        case UP_XF_IN_TREE: return fail(RTMI_ERR_UNSUPPORTED, name, "a record of a primitive inside a BVH item: its boxes depend on it");
        case UP_XF_GROUP: return fail(RTMI_ERR_UNSUPPORTED, name, "a record of a deferred group");
        default: return fail(RTMI_ERR_INVALID, name, "a record outside every transform chain");
        }
    }
    if (int rc = begin_blocking(s)) return rc;
    UPX_TRY(s->up_h_stage.grow((size_t)count * sizeof(rtmi_xform)));
    memcpy(s->up_h_stage.ptr, recs, (size_t)count * sizeof(rtmi_xform));
    const char *staged = reinterpret_cast<const char *>(s->up_h_stage.ptr);
    BusyMark busy{s, s->stream.s};
    UPX_TRY(hipMemcpyAsync(const_cast<rtmi_xform *>(s->dev.xforms) + first, staged, (size_t)count * sizeof(rtmi_xform), hipMemcpyHostToDevice, s->stream.s));
    for (uint32_t k = 0; k < count; k++) { // the copies of an item's first two transforms in its record (DevItem::x0, x1)
        const int32_t i = s->up_xf_item[first + k];
        if (i < 0) continue;
        const DevItem *D = s->dev.items + i;
        const int32_t slot = s->up_xf_slot[first + k];
        if (slot > 1) continue;
        void *dst = const_cast<rtmi_xform *>(slot == 0 ? &D->x0 : &D->x1);
        UPX_TRY(hipMemcpyAsync(dst, staged + (size_t)k * sizeof(rtmi_xform), sizeof(rtmi_xform), hipMemcpyHostToDevice, s->stream.s));
    }
    UPX_TRY(hipStreamSynchronize(s->stream.s));
    return RTMI_OK;
}

extern "C" int rtmu_probe_scene_words(rtmi_scene *s, int which, void *out, size_t cap, size_t *need) {
    const char *name = "rtmu_probe_scene_words";
    if (!s) return fail(RTMI_ERR_INVALID, name, "scene is NULL");
    std::lock_guard<std::mutex> lock(s->mu);
    const rtmi_scene_desc &m = s->meta;
    const void *src = nullptr;
    size_t bytes = 0;
    switch (which) {
    case RTMI_SCENE_WORDS_ITEMS: src = s->dev.items; bytes = (size_t)m.n_items * sizeof(DevItem); break;
    case RTMI_SCENE_WORDS_PRIM_A: src = s->dev.prim_a; bytes = (size_t)m.n_prims * 16; break;
    case RTMI_SCENE_WORDS_PRIM_B: src = s->dev.prim_b; bytes = (size_t)m.n_prims * 16; break;
    case RTMI_SCENE_WORDS_GATE: src = s->dev.gate; bytes = s->dev.gate ? (size_t)m.n_prims * 32 : 0; break;
    case RTMI_SCENE_WORDS_NODES: src = s->dev.nodes; bytes = (size_t)m.n_nodes * sizeof(rtmi_bvh_node); break;
    case RTMI_SCENE_WORDS_ALT_NODES: src = s->dev.nodes4; bytes = s->dev.nodes4 ? (size_t)m.n_alt_nodes * sizeof(rtmi_bvh4_node) : 0; break;
    case RTMI_SCENE_WORDS_LEAF_REC: src = s->dev.leaf_rec; bytes = (size_t)m.n_prims * 80; break;
    case RTMI_SCENE_WORDS_SHADE_PRIM: src = s->dev.shade_prim; bytes = (size_t)m.n_prims * 64; break;
    case RTMI_SCENE_WORDS_XFORMS: src = s->dev.xforms; bytes = (size_t)m.n_xforms * sizeof(rtmi_xform); break;
    default: return fail(RTMI_ERR_INVALID, name, "unknown array");
    }
    if (need) *need = bytes;
    if (!out) return RTMI_OK;
    if (cap < bytes) return fail(RTMI_ERR_INVALID, name, "the buffer is smaller than the array");
    if (bytes == 0) return RTMI_OK;
    RTMI_HIP_TRY("rtmu_probe_scene_words: ", false, hipSetDevice(s->device), "hipSetDevice");
    if (s->busy_recorded) RTMI_HIP_TRY("rtmu_probe_scene_words: ", false, hipEventSynchronize(s->busy.e), "hipEventSynchronize");
    RTMI_HIP_TRY("rtmu_probe_scene_words: ", false, hipMemcpy(out, src, bytes, hipMemcpyDeviceToHost), "hipMemcpy");
    return RTMI_OK;
}
