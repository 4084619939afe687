// TEST INFRASTRUCTURE, computes nothing but containers -- a stand-in for the tps_config.h that the reference's configure
// step generates.  No HAVE_* feature is defined: no GSL (the two-dimensional tables), no MASA, no GPU back end.
#ifndef TPSREF_STUB_TPS_CONFIG_H_
#define TPSREF_STUB_TPS_CONFIG_H_
#define PACKAGE_VERSION "point-physics-checker"
#endif
