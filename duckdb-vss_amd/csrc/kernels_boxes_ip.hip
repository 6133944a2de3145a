// kernels_boxes_ip.hip — the box walkers' instantiations for metric ip (see kernels_boxes.inc)
#define VSS_MT 2
#include "kernels_boxes.inc"
