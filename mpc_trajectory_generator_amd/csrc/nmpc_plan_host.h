// nmpc_plan_host.h -- host side of the route planner on device (its kernels: nmpc_plan.h): struct nmpc_planner and the nmpc_planner_* /
// nmpc_plan_batch_* entry points of include/nmpc_solver.h.  Part of the one translation unit: nmpc_kernels.hip includes it inside its
// extern "C" block, after fail and HIP_TRY.  A planner has no handle, so its errors carry no text (HIP_TRY(nullptr, ..)).
#pragma once

struct nmpc_planner {
    int device = 0, max_batch = 0;
    int V = 0, E = 0, n_poly = 0;
    double last_ms = 0.0;
    DevBuf<double> d_node, d_edge;
    DevBuf<int> d_poff;
    DevBuf<unsigned char> d_nn;          // [V][V]
    DevBuf<unsigned char> d_qvis;        // [max_batch][2V + 1]: a batch's own segments when the caller keeps no copy
    DevBuf<double> d_start, d_goal, d_len;      // the host path's operands
    DevBuf<int> d_nwp, d_wp;
    Event ev[2];
};

static constexpr int PLAN_MAX_BATCH = 1 << 20;      // max_batch * (2V + 1) segments are counted in an int

static void launch_visible(const nmpc_planner *pl, int n_seg, bool queries, const double *d_start, const double *d_goal,
                           unsigned char *out, hipStream_t s)
{
    nmpc::PlanVisArgs a{pl->V, pl->E, pl->n_poly, n_seg, queries ? 1 : 0, pl->d_node, pl->d_edge, pl->d_poff, d_start, d_goal, out};
    const int blocks = (n_seg + nmpc::PLAN_VIS_BLOCK - 1) / nmpc::PLAN_VIS_BLOCK;
    hipLaunchKernelGGL(nmpc::nmpc_plan_visible_kernel, dim3(blocks), dim3(nmpc::PLAN_VIS_BLOCK), 0, s, a);
}

void nmpc_planner_free(nmpc_planner *pl)
{
    if (!pl) return;
    (void)hipSetDevice(pl->device);
    delete pl;
}

int nmpc_planner_new(const nmpc_scene *sc, int device_id, int max_batch, nmpc_planner **out)
{
    if (!sc || !out || max_batch < 1 || max_batch > PLAN_MAX_BATCH) return NMPC_ERR_BAD_ARG;
    const int V = sc->n_node, E = sc->n_edge, np = sc->n_poly;
    if (V < 0 || V > nmpc::PLAN_MAX_NODES || E < 3 || E > nmpc::PLAN_MAX_EDGES || np < 1 || np > nmpc::PLAN_MAX_POLYS ||
        !sc->edge || !sc->poly_off || (V > 0 && !sc->node_xy))
        return NMPC_ERR_BAD_ARG;
    if (sc->poly_off[0] != 0 || sc->poly_off[np] != E) return NMPC_ERR_BAD_ARG;
    for (int k = 0; k < np; ++k)
        if (sc->poly_off[k + 1] - sc->poly_off[k] < 3 || sc->poly_off[k + 1] > E) return NMPC_ERR_BAD_ARG;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device_id < 0 || device_id >= ndev) return NMPC_ERR_NO_DEVICE;
    // (a return below releases what the planner holds so far)
    std::unique_ptr<nmpc_planner, decltype(&nmpc_planner_free)> pl(new nmpc_planner(), nmpc_planner_free);
    pl->device = device_id; pl->max_batch = max_batch; pl->V = V; pl->E = E; pl->n_poly = np;
    const size_t B = (size_t)max_batch, per = 2 * (size_t)V + 1;
    HIP_TRY(nullptr, hipSetDevice(device_id));
    if (V > 0) HIP_TRY(nullptr, pl->d_node.upload(sc->node_xy, 2 * (size_t)V));
    else HIP_TRY(nullptr, pl->d_node.alloc(2));
    HIP_TRY(nullptr, pl->d_edge.upload(sc->edge, 4 * (size_t)E));
    HIP_TRY(nullptr, pl->d_poff.upload(sc->poly_off, (size_t)np + 1));
    HIP_TRY(nullptr, pl->d_nn.alloc((size_t)(V > 0 ? V * V : 1)));
    HIP_TRY(nullptr, pl->d_qvis.alloc(B * per));
    HIP_TRY(nullptr, pl->d_start.alloc(2 * B));
    HIP_TRY(nullptr, pl->d_goal.alloc(2 * B));
    HIP_TRY(nullptr, pl->d_len.alloc(B));
    HIP_TRY(nullptr, pl->d_nwp.alloc(B));
    HIP_TRY(nullptr, pl->d_wp.alloc(B * (size_t)(V + 2)));
    for (int i = 0; i < 2; ++i) HIP_TRY(nullptr, pl->ev[i].create());
    if (V > 0) {
        launch_visible(pl.get(), V * V, false, nullptr, nullptr, pl->d_nn, nullptr);
        HIP_TRY(nullptr, hipGetLastError());
    }
    HIP_TRY(nullptr, hipDeviceSynchronize());
    *out = pl.release();
    return NMPC_OK;
}

double nmpc_planner_last_ms(const nmpc_planner *pl) { return pl ? pl->last_ms : 0.0; }

int nmpc_planner_visibility(nmpc_planner *pl, uint8_t *vis)
{
    if (!pl || !vis) return NMPC_ERR_BAD_ARG;
    HIP_TRY(nullptr, hipSetDevice(pl->device));
    if (pl->V > 0) HIP_TRY(nullptr, pl->d_nn.read(vis, (size_t)pl->V * pl->V));
    return NMPC_OK;
}

int nmpc_plan_batch_device(nmpc_planner *pl, int B, const double *d_start, const double *d_goal, int32_t *d_n_wp, int32_t *d_wp,
                           double *d_length, uint8_t *d_vis, void *stream)
{
    if (!pl || B < 0 || B > pl->max_batch) return NMPC_ERR_BAD_ARG;
    if (B == 0) return NMPC_OK;
    if (!d_start || !d_goal || !d_n_wp || !d_wp || !d_length) return NMPC_ERR_BAD_ARG;
    HIP_TRY(nullptr, hipSetDevice(pl->device));
    hipStream_t s = (hipStream_t)stream;
    unsigned char *vis = d_vis ? d_vis : pl->d_qvis.p;
    launch_visible(pl, B * (2 * pl->V + 1), true, d_start, d_goal, vis, s);
    HIP_TRY(nullptr, hipGetLastError());
    nmpc::PlanPathArgs a{pl->V, pl->d_node, pl->d_nn, d_start, d_goal, vis, d_n_wp, d_wp, d_length};
    hipLaunchKernelGGL(nmpc::nmpc_plan_path_kernel, dim3(B), dim3(64), 0, s, a);
    HIP_TRY(nullptr, hipGetLastError());
    return NMPC_OK;
}

int nmpc_plan_batch_host(nmpc_planner *pl, int B, const double *start, const double *goal, int32_t *n_wp, int32_t *wp, double *length,
                         uint8_t *vis)
{
    if (!pl || B < 0 || B > pl->max_batch) return NMPC_ERR_BAD_ARG;
    if (B == 0) return NMPC_OK;
    if (!start || !goal || !n_wp || !wp || !length) return NMPC_ERR_BAD_ARG;
    HIP_TRY(nullptr, hipSetDevice(pl->device));
    const size_t n = (size_t)pl->V + 2, per = 2 * (size_t)pl->V + 1;
    HIP_TRY(nullptr, hipMemcpy(pl->d_start, start, 2 * (size_t)B * 8, hipMemcpyHostToDevice));
    HIP_TRY(nullptr, hipMemcpy(pl->d_goal, goal, 2 * (size_t)B * 8, hipMemcpyHostToDevice));
    HIP_TRY(nullptr, hipEventRecord(pl->ev[0], nullptr));
    if (const int rc = nmpc_plan_batch_device(pl, B, pl->d_start, pl->d_goal, pl->d_nwp, pl->d_wp, pl->d_len, nullptr, nullptr)) return rc;
    HIP_TRY(nullptr, hipEventRecord(pl->ev[1], nullptr));
    HIP_TRY(nullptr, hipEventSynchronize(pl->ev[1]));
    float ms = 0.f;
    HIP_TRY(nullptr, hipEventElapsedTime(&ms, pl->ev[0], pl->ev[1]));
    pl->last_ms = ms;
    HIP_TRY(nullptr, pl->d_nwp.read(n_wp, B));
    HIP_TRY(nullptr, pl->d_wp.read(wp, (size_t)B * n));
    HIP_TRY(nullptr, pl->d_len.read(length, B));
    HIP_TRY(nullptr, pl->d_qvis.read(vis, (size_t)B * per));
    return NMPC_OK;
}
