// kernels_setboxes_ip.hip — the set-box walkers' instantiations for metric ip (see kernels_setboxes.inc)
#define VSS_MT 2
#include "kernels_setboxes.inc"
