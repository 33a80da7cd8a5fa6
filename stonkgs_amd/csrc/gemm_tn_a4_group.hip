// Grouped instance of the four-wave weight-gradient kernel (stonk_gemm_tn_bf16_group): gemm_tn_a4.hip compiled with a table
// of problems for its argument block and the accumulating epilogue. A translation unit of its own, like the store
// instances, so that the objects of the other three kernels are exactly what they were.
#define STONK_TN_A4_GROUP 1
#include "gemm_tn_a4.hip"
