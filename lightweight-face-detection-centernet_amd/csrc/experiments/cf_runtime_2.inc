// experiments build only (make EXP=1): cut out of cf_runtime.hip -- measured 2-8 % slower than the free-running pair of contexts (DESIGN.md section 4): not in the release library
// ---- two-lane schedule (VERDICT r02 next-8, experimental): the forward is cut into three segments -- front A (stem .. the
// op before cut 1), front B (cut 1 .. the op before cut 2) and the back half (cut 2 .. heads).  With two contexts alternating
// batches, cf_forward_lanes(cur, prev, ...) enqueues
//   1. front A of the new batch on cur's stream, after prev's front B           (front A runs ALONE: it is VALU-bound)
//   2. the back half of prev's batch on prev's stream, after cur's front A      (HBM- / latency-bound, small grids)
//   3. front B of the new batch on cur's stream                                 (runs UNDERNEATH 2: the mid-size kernels)
// so which kernels share the chip is fixed by events instead of by how two free-running chains happen to line up.  prev's
// results are complete after this call's work (decode it now); cf_forward_lanes_flush(c) launches a back half that has no
// successor (end of stream, fences).  Eager launches (no graph): the segments are tens of microseconds each at any batch.
static int lane_cuts(cf_ctx* c) {
    if (c->lane_cut1 >= 0) return CF_OK;
    const char* n1 = getenv("CF_LANE_CUT1") ? getenv("CF_LANE_CUT1") : "layer2.0";      // (experiments build only: this whole section)
    const char* n2 = getenv("CF_LANE_CUT2") ? getenv("CF_LANE_CUT2") : "layer4.0";
    int c1 = -1, c2 = -1;
    for (size_t i = 0; i < c->ops.size(); ++i) {
        if (c->ops[i].fused_away) continue;
        if (c1 < 0 && c->ops[i].name.rfind(n1, 0) == 0) c1 = (int)i;
        if (c2 < 0 && c->ops[i].name.rfind(n2, 0) == 0) c2 = (int)i;
    }
    if (c1 < 0 || c2 < 0 || c1 > c2) return c->fail(CF_EINVAL, "cf_forward_lanes: cut points %s / %s not found in the plan", n1, n2);
    c->lane_cut1 = c1; c->lane_cut2 = c2;
    if (!c->ev_seg1) HIPCHK(c, hipEventCreateWithFlags(&c->ev_seg1, hipEventDisableTiming));
    if (!c->ev_seg2) HIPCHK(c, hipEventCreateWithFlags(&c->ev_seg2, hipEventDisableTiming));
    return CF_OK;
}
static int launch_range(cf_ctx* c, int lo, int hi, const void* net_in, int in_format, int B) {
    for (int i = lo; i < hi; ++i) {
        const Op& op = c->ops[i];
        if (op.fused_away) continue;
        if (op.kind == OP_HEAD && c->dec_pending) {       // the overlapped decode of the batch before still reads heads / hm_plane
            HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_dec, 0));
            c->dec_pending = false;
        }
        HIPCHK(c, launch_op(c, op, net_in, in_format, B));
    }
    return CF_OK;
}
static int lane_back_half(cf_ctx* p) {
    int r = launch_range(p, p->lane_cut2, (int)p->ops.size(), p->lane_in, p->lane_fmt, p->lane_B);
    if (r) return r;
    HIPCHK(p, hipEventRecord(p->ev_fwd, p->stream));
    p->lane_pending = false;
    p->last_B = p->lane_B;
    return CF_OK;
}

int cf_forward_lanes(cf_ctx* cur, cf_ctx* prev, const void* in, int in_format, int in_on_device, int B) {
    if (!cur || cur == prev) return CF_EINVAL;
    if (prev && prev->device != cur->device) return cur->fail(CF_EINVAL, "cf_forward_lanes: both contexts must live on one device");
    if (cur->flip) return cur->fail(CF_ESTATE, "cf_forward_lanes while flip test is on (cf_set_flip_test): it runs the plan of one batch");
    int r = lane_cuts(cur); if (r) return r;
    if (cur->lane_pending) { r = lane_back_half(cur); if (r) return r; }       // its own earlier batch never got a successor
    const void* net_in = nullptr;
    r = stage_input(cur, in, in_format, in_on_device, B, &net_in);
    if (r) return r;
    static const bool alone = cf_ab_int("CF_LANE_ALONE", 1) != 0;        // A/B: front A may overlap prev's front B
    if (alone && prev && prev->seg2_recorded) HIPCHK(cur, hipStreamWaitEvent(cur->stream, prev->ev_seg2, 0));
    r = launch_range(cur, 0, cur->lane_cut1, net_in, in_format, B); if (r) return r;
    HIPCHK(cur, hipEventRecord(cur->ev_seg1, cur->stream));
    r = in_slot_done(cur); if (r) return r;             // the stem has read the host-input slot
    if (prev && prev->lane_pending) {
        HIPCHK(prev, hipSetDevice(prev->device));
        HIPCHK(prev, hipStreamWaitEvent(prev->stream, cur->ev_seg1, 0));
        r = lane_back_half(prev); if (r) return r;
    }
    r = launch_range(cur, cur->lane_cut1, cur->lane_cut2, net_in, in_format, B); if (r) return r;
    HIPCHK(cur, hipEventRecord(cur->ev_seg2, cur->stream));
    cur->seg2_recorded = true;
    cur->lane_pending = true; cur->lane_in = net_in; cur->lane_fmt = in_format; cur->lane_B = B;
    cur->last_B = 0;                                    // no decodable result on cur until its back half has been launched
    return CF_OK;
}

int cf_forward_lanes_flush(cf_ctx* c) {
    if (!c) return CF_EINVAL;
    if (!c->lane_pending) return CF_OK;
    HIPCHK(c, hipSetDevice(c->device));
    return lane_back_half(c);
}
