// rtmi_path_scan.inc — world.hit of one lane's ray: the scan of the top-level list with its BVHs, instances, constant media
// and the deferred / nested / list-scan media rules of rtmi.h.  Included under `need` by the per-lane render body
// (rtmi_kernel_perlane.inc) and by the ray-query kernel (rtmi_query.hip), so both trace a ray with the same text.
// The including code provides FAST and PROF, sc, the ray `pa` (ro, rd, rtime), the lane's traversal stack `stack`, its
// Philox state `g` under the key (k0, k1), `prof`, the results closest, best_item, best_pf and best_medium, and the
// interval as RTMI_SCAN_T_MIN and RTMI_SCAN_T_MAX: the render's (P.t_min, RTMI_FLT_MAX), a query ray's own.  Media
// query their boundaries over (-RTMI_FLT_MAX, RTMI_FLT_MAX) whatever the interval (medium.rs:30-31).
                // ---- world.hit(ray, 0.001, f64::MAX): scan of the top-level list (hittable.rs:37-47)
                RayF W;
                W.o = pa.ro; W.d = pa.rd;
                ray_derive(W);
                closest = RTMI_SCAN_T_MAX;
                best_item = -1; best_pf = 0; best_medium = false;
                float t0_saved = RTMI_FLT_MAX; // the closest hit before a BVH item whose media / instanced-subtree children follow as DEFERRED items
                int grp_first = 0x7fffffff;    // ... the index of that item (or of the first deferred one), and whether it is the enclosing tree
                bool grp_tree = false;
                ListScan ls; // a list with media that was a child of a BVHNode (rtmi.h, LISTSCAN)
                ls.cl = RTMI_FLT_MAX; ls.item = -1; ls.pf = 0; ls.medium = false; ls.has = false;
                for (uint32_t it = 0; it < sc.n_items; it++) {
                    const rtmi_item I = sc.items[it].it;
                    if (I.flags & RTMI_ITEMFLAG_SAVE_T0) {
                        t0_saved = closest; grp_first = (int)it; grp_tree = I.kind == RTMI_ITEM_BVH && !(I.flags & RTMI_ITEMFLAG_DEFERRED);
                    }
                    if (I.flags & RTMI_ITEMFLAG_LISTSCAN_END) { // the terminator: the scan's result meets the closest hit so far
                        listscan_fold(ls, I.first, closest, best_item, best_pf, best_medium, grp_first, grp_tree);
                        continue;
                    }
                    if (I.flags & RTMI_ITEMFLAG_LISTSCAN_BEGIN) { ls.cl = t0_saved; ls.has = false; }
                    const bool scan = (I.flags & RTMI_ITEMFLAG_LISTSCAN_MEMBER) != 0u;
                    RayF R = W;
                    if (I.xform_count > 0) {
                        if (xform_ray(sc.xforms, I.xform_first, I.xform_count, R.o, R.d)) ray_derive(R);
                    }
                    const int slot = 1 + (it < 11u ? (int)it : 11);
                    if (!(I.flags & RTMI_ITEMFLAG_MEDIUM)) {
                        float t;
                        int pf;
                        if (scan) { // a primitive member of the list scan: t_max = the scan's closest hit so far
                            if (deferred_gate(sc, I, W, RTMI_SCAN_T_MIN, t0_saved) &&
                                geom_query<FAST, PROF>(sc, I, R, pa.rtime, RTMI_SCAN_T_MIN, ls.cl, stack, t, pf, prof, slot)) {
                                ls.cl = t; ls.item = (int)it; ls.pf = pf; ls.medium = false; ls.has = true;
                            }
                        } else if (I.flags & RTMI_ITEMFLAG_DEFERRED) { // an instanced subtree that was a child of a BVHNode (rtmi.h)
                            if (deferred_gate(sc, I, W, RTMI_SCAN_T_MIN, t0_saved) &&
                                geom_query<FAST, PROF>(sc, I, R, pa.rtime, RTMI_SCAN_T_MIN, t0_saved, stack, t, pf, prof, slot) &&
                                deferred_bvh_wins(I.count, t, closest, best_item, best_pf, grp_first, grp_tree)) {
                                closest = t; best_item = (int)it; best_pf = pf; best_medium = false;
                            }
                        } else if (geom_query<FAST, PROF>(sc, I, R, pa.rtime, RTMI_SCAN_T_MIN, closest, stack, t, pf, prof, slot)) {
                            closest = t; best_item = (int)it; best_pf = pf; best_medium = false;
                        }
                    } else {
                        // ConstantMedium::hit — medium.rs:28-56
                        float t1, t2, tm;
                        int pf;
                        // a medium that was a child of a BVHNode (rtmi.h, DEFERRED): reached through its parent's box, its
                        // interval clamped to the t_max the BVH was entered with, accepted when closer than the tree's hit
                        const bool dfr = (I.flags & RTMI_ITEMFLAG_DEFERRED) != 0u;
                        const float qmax = scan ? ls.cl : (dfr ? t0_saved : closest);
                        if (!dfr || deferred_gate(sc, I, W, RTMI_SCAN_T_MIN, t0_saved)) {
                        if (geom_query<FAST, PROF>(sc, I, R, pa.rtime, -RTMI_FLT_MAX, RTMI_FLT_MAX, stack, t1, pf, prof, slot)) {
                            if (geom_query<FAST, PROF>(sc, I, R, pa.rtime, t1 + 0.0001f, RTMI_FLT_MAX, stack, t2, pf, prof, slot)) {
                                const float dn = medium_dir_norm(sc, I.flags, I.xform_first, W);
                                if ((I.flags & RTMI_ITEMFLAG_NESTED_MEDIUM) && !nested_medium_interval(sc, I, dn, g, k0, k1, t1, t2)) {
                                    // the inner medium returned no hit to one of the outer medium's two queries
                                } else
                                if (medium_sample(t1, t2, RTMI_SCAN_T_MIN, qmax, dn, I.neg_inv_density, g, k0, k1, tm)) {
                                    if (scan) { ls.cl = tm; ls.item = (int)it; ls.medium = true; ls.has = true; }
                                    else if (!dfr || tm < closest) { closest = tm; best_item = (int)it; best_medium = true; }
                                }
                            }
                        }
                        }
                    }
                }
