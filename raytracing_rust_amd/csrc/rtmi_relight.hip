// rtmi_relight.hip — host unit of the following lights (include/rtmi_relight.h): the entry points and the
// tables a handle builds when following is turned on.  No kernel here, and no launch either: the relight kernel is enqueued
// by an update (enqueue() in rtmi_update.hip, through rtmi_relight_launch.hpp).  rtml_relight_desc is the host evaluation
// of rtmi_relight.hpp and touches no device.
#include "rtmi_host.hpp"

#include <algorithm>
#include <cstddef>

#include "rtmi_light_tree.h"
#include "rtmi_relight.h"
#include "rtmi_relight.hpp"
#include "rtmi_update.h"

#define RLT_TRY(expr) RTMI_HIP_TRY("rtml_scene_follow_lights: ", false, expr, #expr)

static_assert(sizeof(NeeLight) == 48 && offsetof(NeeLight, k) == 16 && offsetof(NeeLight, plane) == 20 && offsetof(NeeLight, prim) == 28 &&
                  offsetof(NeeLight, area) == 32 && offsetof(NeeLight, p_sel) == 36 && offsetof(NeeLight, cdf) == 40,
              "the relight kernel reads a light as twelve words");
static_assert(sizeof(rtmi_light_node) == 32 && offsetof(rtmi_light_node, power) == 16 && offsetof(rtmi_light_node, link) == 20,
              "the relight kernel reads a node as eight words");

extern "C" int rtml_relight_desc(const rtmi_scene_desc *desc, rtmi_light *lights, uint32_t n_lights, void *nodes, uint32_t n_nodes) {
    std::string err;
    const int rc = relight_desc(desc, lights, n_lights, static_cast<rtmi_light_node *>(nodes), n_nodes, err);
    return rc ? fail(rc, "rtml_relight_desc", err.c_str()) : RTMI_OK;
}

// The handle does not keep its description: the attached table and tree, and what gives a light its weight (the primitive's
// material and that material's texture), are read back from the device once.
static int build_tables(rtmi_scene *s) {
    const char *name = "rtml_scene_follow_lights";
    const rtmi_scene_desc &m = s->meta;
    if (s->busy_recorded) RLT_TRY(hipEventSynchronize(s->busy.e));
    const uint32_t n = s->nee_n, slots = s->has_light_tree ? s->lt_n : 0u;
    std::vector<NeeLight> lights(n);
    std::vector<rtmi_light_node> nodes(slots);
    std::vector<rtmi_prim_meta> meta(m.n_prims);
    std::vector<rtmi_material> mats(m.n_materials);
    std::vector<rtmi_texture> texs(m.n_textures);
    if (n) RLT_TRY(hipMemcpy(lights.data(), s->nee_lights.ptr, (size_t)n * sizeof(NeeLight), hipMemcpyDeviceToHost));
    if (slots) RLT_TRY(hipMemcpy(nodes.data(), s->lt_nodes.ptr, (size_t)slots * sizeof(rtmi_light_node), hipMemcpyDeviceToHost));
    if (!meta.empty()) RLT_TRY(hipMemcpy(meta.data(), s->dev.meta, meta.size() * sizeof(rtmi_prim_meta), hipMemcpyDeviceToHost));
    if (!mats.empty()) RLT_TRY(hipMemcpy(mats.data(), s->dev.mats, mats.size() * sizeof(rtmi_material), hipMemcpyDeviceToHost));
    if (!texs.empty()) RLT_TRY(hipMemcpy(texs.data(), s->dev.texs, texs.size() * sizeof(rtmi_texture), hipMemcpyDeviceToHost));
    s->rl_prim_light.assign(m.n_prims, -1);
    s->rl_plane.assign(n, -1);
    s->rl_weight_h.assign(n, 1.0);
    for (uint32_t i = 0; i < n; i++) {
        const int32_t p = lights[i].prim;
        if (p < 0 || (uint32_t)p >= m.n_prims || lights[i].plane < -1 || lights[i].plane > 2)
            return fail(RTMI_ERR_INVALID, name, "the attached light table names a primitive outside the scene");
        s->rl_prim_light[(size_t)p] = (int32_t)i;
        s->rl_plane[i] = lights[i].plane;
        const int32_t mt = meta[(size_t)p].material; // the weight of nee_lights_of: the largest channel of a SOLID emitter texture, else 1
        if (mt >= 0 && (uint32_t)mt < m.n_materials) {
            const int32_t tx = mats[(size_t)mt].tex;
            if (tx >= 0 && (uint32_t)tx < m.n_textures && texs[(size_t)tx].kind == RTMI_TEX_SOLID)
                s->rl_weight_h[i] = std::max(std::max((double)texs[(size_t)tx].f0, (double)texs[(size_t)tx].f1), (double)texs[(size_t)tx].f2);
        }
    }
    std::vector<uint32_t> words;
    s->rl_n_lvl = 0;
    if (slots) {
        std::string err;
        if (!relight_tree_ok(nodes.data(), slots, n, err)) return fail(RTMI_ERR_INVALID, name, err.c_str());
        std::vector<uint32_t> order, lvl;
        relight_levels(nodes.data(), slots, order, lvl);
        s->rl_n_lvl = (uint32_t)lvl.size() - 1u;
        for (uint32_t o : lvl) words.push_back((uint32_t)lvl.size() + o);
        words.insert(words.end(), order.begin(), order.end());
    }
    if (words.empty()) words.push_back(0u);
    RLT_TRY(s->rl_words.alloc(words.size() * sizeof(uint32_t)));
    RLT_TRY(hipMemcpy(s->rl_words.ptr, words.data(), words.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    RLT_TRY(s->rl_weight.alloc((size_t)(n ? n : 1u) * sizeof(double)));
    if (n) RLT_TRY(hipMemcpy(s->rl_weight.ptr, s->rl_weight_h.data(), (size_t)n * sizeof(double), hipMemcpyHostToDevice));
    RLT_TRY(s->rl_scratch.alloc(((size_t)(n ? n : 1u) + (size_t)slots * 7) * sizeof(double)));
    s->rl_ready = true;
    return RTMI_OK;
}

extern "C" int rtml_scene_follow_lights(rtmi_scene *s, int on) {
    const char *name = "rtml_scene_follow_lights";
    if (!s) return fail(RTMI_ERR_INVALID, name, "scene is NULL");
    if (on) {
        {
            std::lock_guard<std::mutex> lock(s->mu);
            if (!s->has_lights) return fail(RTMI_ERR_INVALID, name, "no lights attached (rtmi_scene_attach_lights)");
            if (s->has_f64) return fail(RTMI_ERR_UNSUPPORTED, name, "the handle has f64 planes attached, which an update would leave stale");
        }
        if (int rc = rtmu_scene_update_prepare(s)) return rc; // the update tables: which primitives emit (takes the mutex itself)
    }
    std::lock_guard<std::mutex> lock(s->mu);
    if (!on) {
        s->rl_on = false;
        return RTMI_OK;
    }
    if (!s->has_lights) return fail(RTMI_ERR_INVALID, name, "no lights attached (rtmi_scene_attach_lights)");
    RLT_TRY(hipSetDevice(s->device));
    if (!s->rl_ready)
        if (int rc = build_tables(s)) return rc;
    s->rl_on = true;
    return RTMI_OK;
}

extern "C" int rtml_probe_light_words(rtmi_scene *s, int which, void *out, size_t cap, size_t *need) {
    const char *name = "rtml_probe_light_words";
    if (!s) return fail(RTMI_ERR_INVALID, name, "scene is NULL");
    std::lock_guard<std::mutex> lock(s->mu);
    const void *src = nullptr;
    size_t bytes = 0;
    switch (which) {
    case RTML_WORDS_LIGHTS: src = s->nee_lights.ptr; bytes = s->has_lights ? (size_t)s->nee_n * sizeof(NeeLight) : 0; break;
    case RTML_WORDS_PRIM_LIGHT: src = s->nee_prim_light.ptr; bytes = s->has_lights ? (size_t)s->meta.n_prims * sizeof(int32_t) : 0; break;
    case RTML_WORDS_TREE_NODES: src = s->lt_nodes.ptr; bytes = s->has_light_tree ? (size_t)s->lt_n * sizeof(rtmi_light_node) : 0; break;
    case RTML_WORDS_TREE_PATHS: src = s->lt_paths.ptr; bytes = s->has_light_tree ? (size_t)(s->lt_n / 2u) * sizeof(rtmi_light_path) : 0; break;
    default: return fail(RTMI_ERR_INVALID, name, "unknown array");
    }
    if (need) *need = bytes;
    if (!out) return RTMI_OK;
    if (cap < bytes) return fail(RTMI_ERR_INVALID, name, "the buffer is smaller than the array");
    if (bytes == 0) return RTMI_OK;
    RTMI_HIP_TRY("rtml_probe_light_words: ", false, hipSetDevice(s->device), "hipSetDevice");
    if (s->busy_recorded) RTMI_HIP_TRY("rtml_probe_light_words: ", false, hipEventSynchronize(s->busy.e), "hipEventSynchronize");
    RTMI_HIP_TRY("rtml_probe_light_words: ", false, hipMemcpy(out, src, bytes, hipMemcpyDeviceToHost), "hipMemcpy");
    return RTMI_OK;
}
