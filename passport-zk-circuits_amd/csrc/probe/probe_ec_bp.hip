// Probe kernels for brainpoolP256r1: probe_ec.hip compiled for curve 1.
#define PZK_EC_CURVE 1
#include "probe_ec.hip"
