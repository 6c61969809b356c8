// CPU export of the group normalisation launch plan (kernels/groupnorm_plan.h): ops/_plan.py sizes
// the workspaces and names the form a shape takes with the very functions the launchers use, and
// tests/test_groupnorm_cpu.py checks them without a GPU.
#include "../kernels/groupnorm_plan.h"

#include "common.h"

namespace gnplan = ttdk::gnplan;
typedef long long ll;

TTD_API(int, ttd_gnplan_valid, (ll N, ll M, ll C, ll G)) { return gnplan::valid(N, M, C, G); }
TTD_API(int, ttd_gnplan_fast_takes, (ll N, ll M, ll C, ll G, int dt)) { return gnplan::fast_takes(N, M, C, G, dt); }
TTD_API(int, ttd_gnplan_max_slabs, ()) { return gnplan::kMaxSlabs; }
TTD_API(ll, ttd_gnplan_max_ws_floats, ()) { return gnplan::kMaxWsFloats; }
TTD_API(int, ttd_gnplan_lanes, (ll C, int fast)) { return gnplan::lanes(C, fast != 0); }
TTD_API(int, ttd_gnplan_rows_per_block, (ll C, int fast)) { return gnplan::rows_per_block(C, fast != 0); }
TTD_API(ll, ttd_gnplan_part_stride, (ll C)) { return gnplan::part_stride(C); }
TTD_API(ll, ttd_gnplan_rows_per_slab, (ll N, ll M, ll C)) { return gnplan::rows_per_slab(N, M, C); }
TTD_API(int, ttd_gnplan_parts, (ll N, ll M, ll C)) { return gnplan::parts(N, M, C); }
TTD_API(void, ttd_gnplan_slab_rows, (ll N, ll M, ll C, int t, ll* r0, ll* r1)) { gnplan::slab_rows(N, M, C, t, r0, r1); }
TTD_API(ll, ttd_gnplan_fwd_ws_floats, (ll N, ll M, ll C)) { return gnplan::fwd_ws_floats(N, M, C); }
TTD_API(ll, ttd_gnplan_bwd_ws_floats, (ll N, ll M, ll C)) { return gnplan::bwd_ws_floats(N, M, C); }
