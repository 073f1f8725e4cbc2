// experiments build only (make EXP=1): cut out of cf_dw.hip::dw_strip_launch -- CF_DW_BAND=1 selects dw_band_kernel when one item per thread and band fits
    {
        static const int band = cf_ab_int("CF_DW_BAND", 0);
        const int nitem = TH * (TW / 4) * g.cpp, nitemA = (TH / 2) * (TW / 4) * g.cpp;
        if (band && nitemA <= threads && nitem - nitemA <= threads && ((size_t)g.nch + 63) / 64 <= 16 * (size_t)(threads / 64)) {
            DwLdsGeom gb = g; dw_set_step(gb, threads);
            set_kernel_tag("void cf::dw_band_kernel<%s, %d, %d, %d, %d>(cf::DwParams, cf::DwLdsGeom, int, int, int)", type_tag<T>(), KS, S, TH, TW);
            return launch_lds<dw_band_kernel<T, KS, S, TH, TW>>(dim3((unsigned)nt), dim3(threads), g.lds_bytes, s, p, gb, ntx, nty, (int)nt);
        }
    }
