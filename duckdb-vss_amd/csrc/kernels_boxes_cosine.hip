// kernels_boxes_cosine.hip — the box walkers' instantiations for metric cosine (see kernels_boxes.inc)
#define VSS_MT 1
#include "kernels_boxes.inc"
