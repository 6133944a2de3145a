// kernels_setboxes_cosine.hip — the set-box walkers' instantiations for metric cosine (see kernels_setboxes.inc)
#define VSS_MT 1
#include "kernels_setboxes.inc"
