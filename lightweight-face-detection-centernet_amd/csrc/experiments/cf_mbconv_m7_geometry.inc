// experiments build only (make EXP=1): cut out of cf_mbconv.hip -- the hook of experiments/cf_mbconv7.hip (MB_SP_DIRECT [10])
    if (dtype == 2 && mb7_geometry(dtype, g, Cin, hid, Cout, k, s)) return g;     // (experiments switch CF_M7=1)
