// experiments build only (make EXP=1): cut out of cf_mbconv3.hip
template <int KS, int JX, int TOH, int TOW, int NW, int T>
static hipError_t xmxt_launch_t(hipStream_t s, const MbParams& p) {
    typedef Mx<KS, JX, TOH, TOW, NW, true> G;
    const int units = ((p.Wout + TOW - 1) / TOW) * ((p.Hout + TOH - 1) / TOH) * p.B;
    dim3 grid((units + T - 1) / T, p.hid / 32, 1), blk(NW * 64);
    set_kernel_tag("void cf::expdw_mxt_kernel<%d, %d, %d, %d, %d, %d>(cf::MbParams)", KS, JX, TOH, TOW, NW, T);
    return launch_lds<expdw_mxt_kernel<KS, JX, TOH, TOW, NW, T>>(grid, blk, G::LDS, s, p);
}
