// scan_wide_ring.hip -- the ring kernels of scan_wide.hip's forms (its header: "Ring form"; scan_forms.h: wide_ring_form): the same
// body with three tile buffers, compiled in a translation unit of their own so that scan_wide.hip's kernels stay the code they
// were measured as.  scan_launch_wide_ring is the launcher (Plan::ring).
#define CRS_WIDE_TU 1
#include "scan_wide.hip"
