// Probe kernels for brainpoolP384r1: probe_ec.hip compiled for curve 3.
#define PZK_EC_CURVE 3
#include "probe_ec.hip"
