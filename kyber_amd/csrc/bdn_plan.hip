// kyb_bdn_plan: the table width and the slices a mask_aggregate call of the pairing suites uses (bdn.cuh's plan, which
// every suite's *_bdn unit follows), and the measurement hook that overrides the slices.  Pure host code: no device is
// touched.
#include "bdn.cuh"
#include "context.h"

#include <atomic>

namespace kyb {
static std::atomic<size_t> g_bdn_forced_slices{0};
size_t bdn_forced_slices() { return g_bdn_forced_slices.load(std::memory_order_relaxed); }
}  // namespace kyb

extern "C" int kyb_bdn_debug_set_slices(size_t slices) {
    kyb::g_bdn_forced_slices.store(slices, std::memory_order_relaxed);
    return KYB_OK;
}

extern "C" int kyb_bdn_plan(size_t n, size_t m, int plan[2]) {
    if (n < 1 || m < 1 || m > kyb::BDN_MAX_ROSTER || !plan) {
        kyb::set_error("kyb_bdn_plan: bad argument (n >= 1; 1 <= m <= 8192; plan)");
        return KYB_E_ARG;
    }
    plan[0] = kyb::bdn_group_width(n, m);
    plan[1] = (int)kyb::bdn_slices(n, m, plan[0]);
    return KYB_OK;
}
