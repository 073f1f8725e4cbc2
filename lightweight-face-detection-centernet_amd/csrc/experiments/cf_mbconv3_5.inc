// experiments build only (make EXP=1): cut out of cf_mbconv3.hip
template <int KS, int JX, int NMB, bool RESID, int TOH, int TOW, bool TAIL16>
static hipError_t fz_launch_t(hipStream_t s, const MbParams& p) {
    typedef Fz<KS, JX, NMB, TOH, TOW, TAIL16> G;
    dim3 grid((p.Wout + TOW - 1) / TOW, (p.Hout + TOH - 1) / TOH, p.B), blk(512);
    set_kernel_tag("void cf::mbconv_mxs_kernel<%d, %d, %d, %s, %d, %d, %s>(cf::MbParams)", KS, JX, NMB, RESID ? "true" : "false", TOH, TOW,
                   TAIL16 ? "true" : "false");
    return launch_lds<mbconv_mxs_kernel<KS, JX, NMB, RESID, TOH, TOW, TAIL16>>(grid, blk, G::LDS, s, p);
}
