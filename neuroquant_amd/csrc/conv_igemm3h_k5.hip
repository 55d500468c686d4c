#define NQ_KS 5
#define NQ_IG3_BUILD 2
#include "conv_igemm3_impl.h"
