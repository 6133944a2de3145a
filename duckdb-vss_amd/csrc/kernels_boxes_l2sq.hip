// kernels_boxes_l2sq.hip — the box walkers' instantiations for metric l2sq (see kernels_boxes.inc)
#define VSS_MT 0
#include "kernels_boxes.inc"
