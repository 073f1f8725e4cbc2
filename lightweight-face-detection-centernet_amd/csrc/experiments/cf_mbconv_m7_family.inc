// experiments build only (make EXP=1): cut out of cf_mbconv.hip -- the family row of experiments/cf_mbconv7.hip (MB_SP_DIRECT [10])
    {MB_SP_DIRECT, DT_SPLIT, mb7_pack, mb7_launch},
