// NZ = 64 instantiation of the register-Cholesky box-QP kernels.
#include "qp_kernels.h"
template struct GqQpRegLaunch<64>;
