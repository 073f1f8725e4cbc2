// experiments build only (make EXP=1): cut out of cf_mbconv3.hip
template <int KS, int JX, int TOH, int TOW, int NW, int R>
static hipError_t xmxr_launch_t(hipStream_t s, const MbParams& p) {
    typedef Mx<KS, JX, TOH, TOW, NW, true> G;
    constexpr int LDS = G::EBYTES + 2 * (G::WXB + G::ATB);
    if ((p.hid / 32) % R) return hipErrorInvalidValue;
    dim3 grid(((p.Wout + TOW - 1) / TOW) * ((p.Hout + TOH - 1) / TOH), p.hid / 32 / R, p.B), blk(NW * 64);
    set_kernel_tag("void cf::expdw_mxr_kernel<%d, %d, %d, %d, %d, %d>(cf::MbParams)", KS, JX, TOH, TOW, NW, R);
    return launch_lds<expdw_mxr_kernel<KS, JX, TOH, TOW, NW, R>>(grid, blk, LDS, s, p);
}
