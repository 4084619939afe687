// TEST INFRASTRUCTURE, computes nothing but containers -- <mfem/general/forall.hpp> of the stand-in: the loop macros live in
// ../../mfem.hpp (MFEM_FORALL is a plain host loop).
#ifndef TPSREF_STUB_FORALL_HPP_
#define TPSREF_STUB_FORALL_HPP_
#include "../../mfem.hpp"
#endif
