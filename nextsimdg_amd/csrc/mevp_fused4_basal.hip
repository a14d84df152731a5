// mevp_fused4_basal.hip -- the BASAL instantiations of the stage-per-wave pipeline (landfast ice, basal.hip): the
// kernels of mevp_fused4.hip that read the fourth coefficient pair and add the seabed stress, launched after a packing that saw a depth
// array.  A translation unit of their own: mevp_fused4.hip, compiled as itself, holds the four instantiations it has always held, and its
// listing is what the resource tests and tools/isa_flops.py read.  Everything -- the kernel, the march, the launcher's strip rule -- is that
// file's text; here it is compiled with BASAL = true behind nsdg_launch_mevp_fused4_basal_ranges.
#define NSDG_FUSED4_BASAL_TU
// the stamped diagnostic build (NSDG_P2P_SPINSTAT) times the kernels without the term: its counters and their readers exist once
#undef NSDG_P2P_SPINSTAT
#include "mevp_fused4.hip"
