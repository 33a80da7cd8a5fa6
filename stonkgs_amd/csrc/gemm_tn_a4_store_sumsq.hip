// Store-mode instance of the four-wave weight-gradient kernel that also leaves every output tile's sum of squares
// (stonk_gemm_tn_bf16_store_sumsq): gemm_tn_a4.hip compiled with the third form of its epilogue. A translation unit of its
// own, like gemm_tn_a4_store.hip, so that the objects of the accumulating and the plain store kernel are exactly what they
// were.
#define STONK_TN_A4_STORE 2
#include "gemm_tn_a4.hip"
