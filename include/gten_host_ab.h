/*
 * gten_host_ab.h -- what the decoder of a model or of a batch chose among the device library's A/B forms (include/gten_hip_oplanes.h);
 * exported by libgten_host.so (host/capi_resident.cpp, the one host unit that names the device's A/B headers) beside include/gten_host.h.
 */
#ifndef GTEN_HOST_AB_H
#define GTEN_HOST_AB_H

#include "gten_host.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the decoder of a model / of a batch (created by the call if it was not yet): *planes = 1 where its o launch runs as four
 * K-quarter planes, 0 where as one (gten_hip_decoder_o_planes).  0, or -1 */
int gten_host_model_o_planes(gten_host_model* m, int* planes);
int gten_host_batch_o_planes(gten_host_batch* b, int* planes);

#ifdef __cplusplus
}
#endif
#endif
