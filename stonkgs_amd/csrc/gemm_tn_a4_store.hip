// Store-mode instance of the four-wave weight-gradient kernel (stonk_gemm_tn_bf16_store): gemm_tn_a4.hip compiled with
// its epilogue writing instead of accumulating. A translation unit of its own, so that the accumulating kernel's object -
// its register file and scratch are checked from the build products - is exactly what it was.
#define STONK_TN_A4_STORE 1
#include "gemm_tn_a4.hip"
