// Probe kernels for secp224r1: probe_ec.hip compiled for curve 2.
#define PZK_EC_CURVE 2
#include "probe_ec.hip"
