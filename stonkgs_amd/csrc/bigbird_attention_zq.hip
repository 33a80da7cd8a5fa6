// The STONK_BSA_ZERO_MASKED_QUERIES instances of the block-sparse attention kernels (forward, dQ, dK / dV with the query's
// own mask word applied: see the head of bigbird_attention.hip), in an object of their own: bigbird_attention.o keeps the
// kernels it had. The kernels are bigbird_attention.hip's text.
#define STONK_BB_ZQ_UNIT
#include "bigbird_attention.hip"
