// One variant of lin_fused_kernel (lin_fused.h) per translation unit: the fully unrolled k-loops compile in parallel.
#include "lin_fused.h"

template int kpgnn::lin_fused_launch<2, 2>(const kpgnn::LinFParams&, hipStream_t);
