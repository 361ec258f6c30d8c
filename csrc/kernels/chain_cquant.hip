// CQ-GADMM (censored Q-GADMM): the CENS = true instantiations of csrc/kernels/chain_quant.hip --
// chain_phase_linear_cq, chain_persistent_cq_kernel, chain_persistent_cq_sweep_kernel -- and their
// launchers, as a translation unit of their own: compiled next to the Q kernels they changed the Q
// kernels' register allocation, and those are to stay exactly as they were. All code is in
// chain_quant.hip.
#define GADMM_CQ_TU 1
#include "chain_quant.hip"
