# TEST INFRASTRUCTURE.  Builds oracle/_ref/libtpsref_point.so: the point-physics translation units of the REFERENCE,
# compiled by path from its checkout against the stand-in headers of ref_stub/, plus our driver ref_point.cpp.
# Nothing of the reference is copied here and oracle/_ref/ stays out of version control.
#
#   make -C oracle -f ref.mk                 (TPS_REFERENCE_DIR=/path/to/checkout, default /root/reference)
#
# Without a checkout the target does nothing and succeeds; whatever oracle/_ref/ already holds is left alone.
# Flags: reproducible IEEE double -- no contraction into FMAs, no fast-math, no OpenMP; asserts of the reference stay on.
# MPI / HDF5: the reference's headers include <mpi.h> and <hdf5.h> for types only.  Both are taken from the HDF5
# installation the product's own restart library is built against (HDF5_DIR, as in __graft_entry__.build(); an MPI build
# of HDF5 ships mpi.h next to hdf5.h), or from TPSREF_INC.  The one call the units make, MPI_Barrier on an error path, is
# answered by a no-op in ref_point.cpp, so no library of either is linked.
CXX ?= g++
TPS_REFERENCE_DIR ?= /root/reference
HDF5_DIR ?= /opt/conda
TPSREF_INC ?= $(HDF5_DIR)/include
REFSRC := $(TPS_REFERENCE_DIR)/src
REFFLAGS := -MMD -MP -O2 -ffp-contract=off -std=c++17 -fPIC -w -Iref_stub -I$(TPSREF_INC) -I$(REFSRC)
UNITS := equation_of_state transport_properties gas_transport collision_integrals chemistry reaction table radiation \
         fluxes riemann_solver lte_mixture
OBJS := $(UNITS:%=_ref/obj/%.o)
STUBS := ref_stub/mfem.hpp ref_stub/mfem/general/forall.hpp ref_stub/grvy.h ref_stub/tps_config.h
OUT := _ref/libtpsref_point.so

ifeq ($(wildcard $(REFSRC)/equation_of_state.cpp),)
all:
	@echo "oracle/ref.mk: no reference checkout at $(TPS_REFERENCE_DIR): libtpsref_point.so not built"
else
all: $(OUT)
endif

_ref/obj/%.o: $(REFSRC)/%.cpp $(STUBS)
	@mkdir -p _ref/obj
	$(CXX) $(REFFLAGS) -c $< -o $@

_ref/obj/ref_point.o: ref_point.cpp $(STUBS) ../include/tpsrhs.h
	@mkdir -p _ref/obj
	$(CXX) $(REFFLAGS) -Wall -Wno-unused-parameter -I../include -c $< -o $@

$(OUT): $(OBJS) _ref/obj/ref_point.o
	$(CXX) -shared -o $@ $^ -Wl,--no-undefined

# what every object really read (the reference's own headers among it): a change in the checkout rebuilds
-include $(OBJS:.o=.d) _ref/obj/ref_point.d

.PHONY: all
