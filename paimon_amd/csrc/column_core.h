// Element widths of the column dtypes (enum pmh_dtype, include/paimon_hip.h):
// the one definition shared by the host staging code (plan.cpp) and the emit
// kernels (kernels.hip). constexpr, so both sides check it at compile time.
#ifndef PMH_COLUMN_CORE_H
#define PMH_COLUMN_CORE_H

#include "../../include/paimon_hip.h"

// bytes per element of an OUTPUT column; 0 = not a plan column dtype
constexpr int pmh_out_width(int dt) {
    switch (dt) {
    case PMH_DT_INT8: return 1;
    case PMH_DT_INT16: return 2;
    case PMH_DT_INT32:
    case PMH_DT_FLOAT32:
    case PMH_DT_STRING: return 4;  // strings: global dictionary ids
    case PMH_DT_INT64:
    case PMH_DT_FLOAT64: return 8;
    }
    return 0;
}

// bytes per element of a STAGED column: the parquet physical widths
// (INT8/16/32 are stored as INT32; the string id streams decode to int32)
constexpr int pmh_stored_width(int dt) {
    return pmh_out_width(dt) == 8 ? 8 : pmh_out_width(dt) ? 4 : 0;
}

static_assert(pmh_out_width(PMH_DT_INT8) == 1 &&
                  pmh_out_width(PMH_DT_INT16) == 2 &&
                  pmh_out_width(PMH_DT_INT32) == 4 &&
                  pmh_out_width(PMH_DT_INT64) == 8 &&
                  pmh_out_width(PMH_DT_FLOAT32) == 4 &&
                  pmh_out_width(PMH_DT_FLOAT64) == 8 &&
                  pmh_out_width(PMH_DT_STRING) == 4 &&
                  pmh_out_width(PMH_DT_BOOL) == 0 && pmh_out_width(0) == 0,
              "output widths");
static_assert(pmh_stored_width(PMH_DT_INT8) == 4 &&
                  pmh_stored_width(PMH_DT_INT16) == 4 &&
                  pmh_stored_width(PMH_DT_INT32) == 4 &&
                  pmh_stored_width(PMH_DT_INT64) == 8 &&
                  pmh_stored_width(PMH_DT_FLOAT32) == 4 &&
                  pmh_stored_width(PMH_DT_FLOAT64) == 8 &&
                  pmh_stored_width(PMH_DT_STRING) == 4 &&
                  pmh_stored_width(PMH_DT_BOOL) == 0 &&
                  pmh_stored_width(0) == 0,
              "stored widths");

#endif  // PMH_COLUMN_CORE_H
