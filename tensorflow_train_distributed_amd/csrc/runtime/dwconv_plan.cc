// CPU export of the depthwise convolution launch plan (kernels/dwconv_plan.h): ops/_plan.py sizes
// the weight-gradient workspace and names the form a shape takes with the very functions the
// launchers use, and tests/test_depthwise_cpu.py checks them without a GPU.
#include "../kernels/dwconv_plan.h"

#include "common.h"

namespace dwplan = ttdk::dwplan;

TTD_API(int, ttd_dwplan_geom_size, ()) { return static_cast<int>(sizeof(TtdkDwConv)); }
TTD_API(int, ttd_dwplan_valid, (const TtdkDwConv* g)) { return dwplan::valid(*g); }
TTD_API(int, ttd_dwplan_fast_takes, (const TtdkDwConv* g, int dt)) { return dwplan::fast_takes(*g, dt); }
TTD_API(int, ttd_dwplan_strip, ()) { return dwplan::kStrip; }
TTD_API(int, ttd_dwplan_max_slabs, ()) { return dwplan::kMaxSlabs; }
TTD_API(int, ttd_dwplan_wgrad_parts, (const TtdkDwConv* g)) { return dwplan::wgrad_parts(*g); }
TTD_API(void, ttd_dwplan_slab_rows, (const TtdkDwConv* g, int t, long long* r0, long long* r1)) {
  dwplan::slab_rows(*g, t, r0, r1);
}
TTD_API(long long, ttd_dwplan_part_stride, (const TtdkDwConv* g)) { return dwplan::part_stride(*g); }
TTD_API(long long, ttd_dwplan_wgrad_ws_floats, (const TtdkDwConv* g)) { return dwplan::wgrad_ws_floats(*g); }
