// Third translation unit of hn_field2_obj.hip: the evaluation kernels of HN_PREC_F16 (k_field2_obj_f16<MODE>: hidden layers
// on one f16 MFMA per product instead of three), compiled beside the f16x3 kernels.
#define HN_OBJ_F16_TU 1
#include "hn_field2_obj.hip"
