// Document-masked causal attention: toa_attn_fwd_doc / toa_attn_bwd_doc and
// the DOC instantiations of attention.hip's register-staged kernels, in a
// translation unit -- and so a device code object -- of their own.  A process
// that never asks for a mask never loads it, and attention.hip's own code
// object holds exactly the kernels of the unmasked paths.
#define TOA_ATTN_DOC_TU 1
#include "attention.hip"
