#define NQ_KS 3
#define NQ_IG3_BUILD 1
#include "conv_igemm3_impl.h"
