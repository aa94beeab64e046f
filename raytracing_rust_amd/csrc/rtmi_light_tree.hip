// rtmi_light_tree.hip — translation unit of the light tree (include/rtmi_light_tree.h): the NEE kernel that selects its
// light by walking the tree, the probe kernel, their launchers, the host build of the tree and the host form of the walks.
// Compiled with the flags of rtmi_device.hip (-ffp-contract=off: no fused operations, so numpy restates the walks bit for
// bit, and the host functions below compute what the kernels compute).
//
// The kernel is rtmi_nee_kernel (rtmi_nee.hip) with RTMI_PATH_TREE: phase B's shade_hit<.., NEE, ENV = false, TREE = true>
// takes the light of a vertex from light_tree_pick and weights a BSDF hit of a light with light_tree_pmf (rtmi_shade.hpp).
// A lane's walk is a dependent chain of at most ceil(log2 n) reads of one aligned 64-B child pair (four 16-B loads).
// Instantiated for FAST x SIG.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "rtmi.h"
#include "rtmi_math.h"
#include "rtmi_light_tree.h"

#define RTMI_LEAN_TU 1 /* the plain kernels are defined in rtmi_device.hip */
#include "rtmi_kernels.hpp"
#include "rtmi_light_launch.hpp"
#include "rtmi_hostkit.hpp"

static_assert(sizeof(rtmi_light_node) == 32 && sizeof(rtmi_light_path) == 8, "light tree layout");

#define RTMI_PATH_TREE 1
template <bool FAST, bool SIG>
__global__ __launch_bounds__(64 * WAVES_PER_BLOCK) void rtmi_nee_tree_kernel(DevScene sc, DevCamera cam, DevParams P, DevLights nl,
                                                                             DevLightTree lt) {
    constexpr bool PROF = false, TILE_LIST = false, FEATURES = false, NEE = true, ENV = false;
    const DevEnv ev{};
    const uint32_t *const tiles = nullptr;
#include "rtmi_kernel_perlane.inc"
}
#undef RTMI_PATH_TREE

hipError_t rtmi_light_tree_launch_render(bool fast, bool sig, uint32_t blocks, hipStream_t stream, const DevScene &sc,
                                         const DevCamera &cam, const DevParams &P, const DevLights &L, const DevLightTree &T) {
    const dim3 grid(blocks), block(64 * WAVES_PER_BLOCK);
    return rtmi_with_bools([&](auto FAST, auto SIG) {
        hipLaunchKernelGGL((rtmi_nee_tree_kernel<FAST(), SIG()>), grid, block, 0, stream, sc, cam, P, L, T);
        return hipGetLastError();
    }, fast, sig);
}

// one walk per thread: PICK reads a uniform and writes the light and its probability, PMF reads a light (the host has
// checked it against the table) and writes its probability
__global__ __launch_bounds__(256) void rtmi_light_tree_probe_kernel(int op, DevLightTree T, const float *__restrict__ points,
                                                                   const uint32_t *__restrict__ aux, uint32_t n,
                                                                   uint32_t *__restrict__ out_light, float *__restrict__ out_p) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const float x = points[3 * (size_t)k], y = points[3 * (size_t)k + 1], z = points[3 * (size_t)k + 2];
    if (op == RTMI_LIGHT_TREE_PROBE_PICK) {
        float p;
        out_light[k] = light_tree_pick(T.nodes, x, y, z, __uint_as_float(aux[k]), p);
        out_p[k] = p;
    } else {
        out_p[k] = light_tree_pmf(T.nodes, T.paths[aux[k]], x, y, z);
    }
}

hipError_t rtmi_light_tree_launch_probe(int op, const DevLightTree &T, const float *points, const uint32_t *aux, uint32_t n,
                                        uint32_t *out_light, float *out_p, hipStream_t stream) {
    if (n == 0u) return hipSuccess;
    hipLaunchKernelGGL(rtmi_light_tree_probe_kernel, dim3((n + 255u) / 256u), dim3(256), 0, stream, op, T, points, aux, n, out_light,
                       out_p);
    return hipGetLastError();
}

// ---- the host build (include/rtmi_light_tree.h, "The tree") ----------------------------------------------------------------
namespace {
struct Box { double lo[3], hi[3]; };
struct TreeBuild {
    const std::vector<Box> &box;
    const std::vector<double> &power;
    std::vector<double> cen; // [light][3]
    std::vector<rtmi_light_node> &nodes;
    std::vector<rtmi_light_path> &paths;

    // fills `slot` with the node over `idx` and everything below it; returns the node's f64 power
    double fill(uint32_t slot, std::vector<uint32_t> &idx, uint32_t depth, uint32_t trail) {
        Box b = box[idx[0]];
        for (size_t k = 1; k < idx.size(); k++)
            for (int a = 0; a < 3; a++) {
                b.lo[a] = std::min(b.lo[a], box[idx[k]].lo[a]);
                b.hi[a] = std::max(b.hi[a], box[idx[k]].hi[a]);
            }
        double h[3];
        for (int a = 0; a < 3; a++) h[a] = (b.hi[a] - b.lo[a]) * 0.5;
        const double r2 = (h[0] * h[0] + h[1] * h[1]) + h[2] * h[2];
        double pw;
        uint32_t link;
        if (idx.size() == 1) {
            pw = power[idx[0]];
            link = RTMI_LIGHT_TREE_LEAF | idx[0];
            paths[idx[0]].trail = trail;
            paths[idx[0]].depth = depth;
        } else {
            double cl[3], ch[3];
            for (int a = 0; a < 3; a++) cl[a] = ch[a] = cen[(size_t)idx[0] * 3 + a];
            for (size_t k = 1; k < idx.size(); k++)
                for (int a = 0; a < 3; a++) {
                    cl[a] = std::min(cl[a], cen[(size_t)idx[k] * 3 + a]);
                    ch[a] = std::max(ch[a], cen[(size_t)idx[k] * 3 + a]);
                }
            int ax = 0;
            if (ch[1] - cl[1] > ch[ax] - cl[ax]) ax = 1;
            if (ch[2] - cl[2] > ch[ax] - cl[ax]) ax = 2;
            std::stable_sort(idx.begin(), idx.end(),
                             [&](uint32_t p, uint32_t q) { return cen[(size_t)p * 3 + ax] < cen[(size_t)q * 3 + ax]; });
            const size_t mid = (idx.size() + 1) / 2;
            std::vector<uint32_t> left(idx.begin(), idx.begin() + mid), right(idx.begin() + mid, idx.end());
            idx.clear();
            idx.shrink_to_fit();
            link = (uint32_t)nodes.size();
            nodes.resize(nodes.size() + 2);
            const double pl = fill(link, left, depth + 1u, trail);
            const double pr = fill(link + 1u, right, depth + 1u, depth < 32u ? trail | (1u << depth) : trail);
            pw = pl + pr;
        }
        rtmi_light_node N;
        for (int a = 0; a < 3; a++) N.c[a] = (float)((b.lo[a] + b.hi[a]) * 0.5);
        N.r2 = (float)r2;
        N.power = (float)pw;
        N.link = link;
        N.pad[0] = N.pad[1] = 0u;
        nodes[slot] = N;
        return pw;
    }
};
} // namespace

// The tree over the light table of `d` (rtmi_lights_from_desc): 2 * lights nodes and one path per light; both empty for an
// empty table.  Host code only.  An RTMI code, with the message of rtmi_last_error.
int rtmi_light_tree_build(const rtmi_scene_desc *d, std::vector<rtmi_light_node> &nodes, std::vector<rtmi_light_path> &paths) {
    nodes.clear();
    paths.clear();
    uint32_t n = 0;
    if (int rc = rtmi_lights_from_desc(d, nullptr, 0, &n)) return rc;
    if (n == 0u) return RTMI_OK;
    if (n > 0x40000000u) return rtmi_fail(RTMI_ERR_INVALID, "rtmi_light_tree_from_desc: more than 2^30 lights");
    std::vector<rtmi_light> L(n);
    if (int rc = rtmi_lights_from_desc(d, L.data(), n, &n)) return rc;
    std::vector<Box> box(n);
    std::vector<double> power(n), cen((size_t)n * 3);
    for (uint32_t i = 0; i < n; i++) {
        const float *A = d->prim_a + (size_t)L[i].prim * 4;
        Box &b = box[i];
        if (L[i].kind == RTMI_PRIM_RECT) { // plane 0 = YZ (a = y, b = z), 1 = ZX (a = z, b = x), 2 = XY (a = x, b = y)
            const int plane = (int)((d->prim_meta[L[i].prim].flags >> RTMI_PRIMFLAG_PLANE_SHIFT) & 3u);
            const int ka = plane == 0 ? 1 : (plane == 1 ? 2 : 0), kb = plane == 0 ? 2 : (plane == 1 ? 0 : 1);
            const int kk = plane == 0 ? 0 : (plane == 1 ? 1 : 2);
            b.lo[ka] = (double)A[0]; b.hi[ka] = (double)A[2];
            b.lo[kb] = (double)A[1]; b.hi[kb] = (double)A[3];
            b.lo[kk] = b.hi[kk] = (double)d->prim_b[(size_t)L[i].prim * 4];
        } else {
            for (int a = 0; a < 3; a++) { b.lo[a] = (double)A[a] - (double)A[3]; b.hi[a] = (double)A[a] + (double)A[3]; }
        }
        for (int a = 0; a < 3; a++) cen[(size_t)i * 3 + a] = (b.lo[a] + b.hi[a]) * 0.5;
        power[i] = L[i].area * L[i].weight;
    }
    nodes.assign(2, rtmi_light_node{});
    nodes.reserve((size_t)2 * n);
    paths.assign(n, rtmi_light_path{});
    std::vector<uint32_t> idx(n);
    for (uint32_t i = 0; i < n; i++) idx[i] = i;
    TreeBuild tb{box, power, std::move(cen), nodes, paths};
    tb.fill(1u, idx, 0u, 0u);
    return RTMI_OK;
}

extern "C" int rtmi_light_tree_from_desc(const rtmi_scene_desc *desc, rtmi_light_node *out, uint32_t cap, uint32_t *n_nodes,
                                         rtmi_light_path *out_paths) {
    if (!desc || !n_nodes || (cap && !out)) return rtmi_fail(RTMI_ERR_INVALID, "rtmi_light_tree_from_desc: NULL argument");
    std::vector<rtmi_light_node> nodes;
    std::vector<rtmi_light_path> paths;
    if (int rc = rtmi_light_tree_build(desc, nodes, paths)) return rc;
    for (size_t i = 0; i < nodes.size() && i < cap; i++) out[i] = nodes[i];
    if (out_paths)
        for (size_t i = 0; i < paths.size() && i < cap / 2u; i++) out_paths[i] = paths[i];
    *n_nodes = (uint32_t)nodes.size();
    return RTMI_OK;
}

// a caller's tree may be anything: every interior link must name a pair inside the array, behind its node (so a walk ends)
static int light_tree_check(const char *name, const rtmi_light_node *nodes, uint32_t n_nodes) {
    if (n_nodes < 2u || (n_nodes & 1u)) return rtmi_fail(RTMI_ERR_INVALID, (std::string(name) + ": n_nodes must be even and >= 2").c_str());
    for (uint32_t i = 1; i < n_nodes; i++) {
        const uint32_t link = nodes[i].link;
        if (link & RTMI_LIGHT_TREE_LEAF) {
            if ((link & 0x7fffffffu) >= n_nodes / 2u) return rtmi_fail(RTMI_ERR_INVALID, (std::string(name) + ": a leaf names a light outside the table").c_str());
        } else if (link <= i || (link & 1u) || link > n_nodes - 2u) {
            return rtmi_fail(RTMI_ERR_INVALID, (std::string(name) + ": a link leaves the array").c_str());
        }
    }
    return RTMI_OK;
}

extern "C" int rtmi_light_tree_pick(const rtmi_light_node *nodes, uint32_t n_nodes, const float *points, const float *us, uint32_t n,
                                    uint32_t *out_light, float *out_p) {
    const char *name = "rtmi_light_tree_pick";
    if (!nodes || (n > 0u && (!points || !us))) return rtmi_fail(RTMI_ERR_INVALID, "rtmi_light_tree_pick: NULL argument");
    if (int rc = light_tree_check(name, nodes, n_nodes)) return rc;
    const float4 *dn = reinterpret_cast<const float4 *>(nodes);
    for (uint32_t k = 0; k < n; k++) {
        float p;
        const uint32_t li = light_tree_pick(dn, points[3 * (size_t)k], points[3 * (size_t)k + 1], points[3 * (size_t)k + 2], us[k], p);
        if (out_light) out_light[k] = li;
        if (out_p) out_p[k] = p;
    }
    return RTMI_OK;
}

extern "C" int rtmi_light_tree_pmf(const rtmi_light_node *nodes, uint32_t n_nodes, const rtmi_light_path *paths, const float *points,
                                   const uint32_t *lights, uint32_t n, float *out_p) {
    const char *name = "rtmi_light_tree_pmf";
    if (!nodes || !paths || (n > 0u && (!points || !lights || !out_p)))
        return rtmi_fail(RTMI_ERR_INVALID, "rtmi_light_tree_pmf: NULL argument");
    if (int rc = light_tree_check(name, nodes, n_nodes)) return rc;
    for (uint32_t k = 0; k < n; k++)
        if (lights[k] >= n_nodes / 2u) return rtmi_fail(RTMI_ERR_INVALID, "rtmi_light_tree_pmf: a light index is outside the table");
    const float4 *dn = reinterpret_cast<const float4 *>(nodes);
    for (uint32_t k = 0; k < n; k++) {
        const rtmi_light_path &pt = paths[lights[k]];
        out_p[k] = light_tree_pmf(dn, make_uint2(pt.trail, pt.depth), points[3 * (size_t)k], points[3 * (size_t)k + 1],
                                  points[3 * (size_t)k + 2]);
    }
    return RTMI_OK;
}
