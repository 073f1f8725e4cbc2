// experiments build only (make EXP=1): cut out of cf_uphead.hip
    static const int var = cf_ab_int("CF_UH_VARIANT", 0);           // A/B sweep of tile height / waves / non-temporal record stores
    if (dtype == 1) {
        if (cf_ab_int("CF_UH_RUNS", 1) == 0) return uphead_launch_t<bf16_t, true, 16, 8, true>(s, q);     // one tile per workgroup
        if (cf_ab_int("CF_UH_COALESCE", 1) == 0) return uphead_launch_t<bf16_t, false, 8, 4, false>(s, q);
        switch (var) {
            case 1: return uphead_launch_t<bf16_t, true, 8, 4, true>(s, q);
            case 2: return uphead_launch_t<bf16_t, true, 16, 8, false>(s, q);
            case 3: return uphead_launch_t<bf16_t, true, 8, 4, false>(s, q);       // the round-3 geometry
            case 4: return uphead_launch_t<bf16_t, true, 16, 4, true>(s, q);
            case 5: return uphead_launch_t<bf16_t, true, 32, 8, true>(s, q);
            case 6: return uphead_launch_t<bf16_t, true, 8, 8, true>(s, q);
            default: break;
        }
    } else if (dtype == 2) {
        switch (var) {
            case 1: return uphead_launch_t<sp32_t, true, 8, 4, true>(s, q);
            case 2: return uphead_launch_t<sp32_t, true, 16, 8, true>(s, q);
            case 3: return uphead_launch_t<sp32_t, true, 4, 4, true>(s, q);
            case 4: return uphead_launch_t<sp32_t, true, 16, 16, true>(s, q);
            default: break;
        }
    }
