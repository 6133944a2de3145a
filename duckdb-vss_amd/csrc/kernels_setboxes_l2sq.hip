// kernels_setboxes_l2sq.hip — the set-box walkers' instantiations for metric l2sq (see kernels_setboxes.inc)
#define VSS_MT 0
#include "kernels_setboxes.inc"
