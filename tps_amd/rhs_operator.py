"""Python image of the reference's ``RHSoperator`` (``src/rhs_operator.hpp:59-235``) over the C ABI.

The class keeps the reference's method names and argument meaning -- ``Mult(x, y)``,
``updatePrimitives``/``updateGradients``, ``getGradients`` -- so that tests read like
``utils/compute_rhs.cpp:60-102`` and ``test/test_gradient.cpp:159-162``.  ``x`` and ``y`` are
torch CUDA tensors (float64, ``num_equation * NDofs``, byNODES); torch is used only to own device
memory and streams.  Everything is computed by ``libtpsrhs.so``; a missing library or a missing
GPU raises -- there is no CPU path.
"""
from __future__ import annotations

import ctypes as C
import weakref

import numpy as np
import torch

from . import capi


class TpsRhsError(RuntimeError):
    def __init__(self, status, where):
        lib = capi.load()
        self.status = status
        msg = lib.tpsrhs_last_error().decode()
        super().__init__(f"{where}: {lib.tpsrhs_status_string(status).decode()}: {msg}")


class RHSoperator:
    """``RHSoperator : mfem::TimeDependentOperator`` -- one instance per rank / per GPU.

    Parameters mirror what ``M2ulPhyS::initVariables`` hands the reference constructor
    (``src/M2ulPhyS.cpp:745-749``): the (local) mesh, the discretisation, the physics parameter
    blocks, the boundary conditions.  ``halo`` is the neighbour-exchange hook used on partitioned
    meshes (see :mod:`tps_amd.halo`).
    """

    def __init__(self, host_mesh, disc, physics, bcs=(), device=0, halo=None, stream=None):
        self._lib = capi.load()
        if not torch.cuda.is_available():
            raise RuntimeError("tps_amd.RHSoperator needs a HIP device (torch.cuda.is_available() is False)")
        self.device = torch.device("cuda", device)
        self._margs = capi.MeshArgs(host_mesh)
        self._disc, self._physics = disc, physics
        self._mesh, self._bc_list = host_mesh, list(bcs)
        self._bcs = (capi.BC * max(1, len(bcs)))(*bcs)
        rt = capi.Runtime()
        rt.device = device
        st = stream if stream is not None else torch.cuda.current_stream(self.device)
        self._stream = st
        rt.stream = C.c_void_p(st.cuda_stream)
        self._halo = halo
        if halo is not None and hasattr(halo, "c_halo"):  # native exchange (tps_amd.halo_rccl): C function pointers
            rt.halo, rt.halo_ctx = halo.c_halo, halo.ctx
            rt.reduce, rt.reduce_ctx = halo.c_reduce, halo.ctx
        elif halo is not None:  # Python hook (tps_amd.halo): gloo rehearsals and tests
            self._halo_cb = capi.HALO_FN(halo.callback)
            rt.halo = self._halo_cb
            if hasattr(halo, "reduce_callback"):
                self._reduce_cb = capi.REDUCE_FN(halo.reduce_callback)
                rt.reduce = self._reduce_cb
        self._rt = rt
        h = C.c_void_p()
        st_code = self._lib.tpsrhs_create(C.byref(self._margs.c), C.byref(disc), C.byref(physics), len(bcs),
                                          self._bcs, C.byref(rt), C.byref(h))
        if st_code != 0:
            raise TpsRhsError(st_code, "tpsrhs_create")
        self._h = h
        self.dim = host_mesh.dim
        self.num_equation = int(self._lib.tpsrhs_num_equation(h))
        self.NDofs = int(self._lib.tpsrhs_num_dofs(h))
        self.max_char_speed = 0.0
        self._time = 0.0

    # -- mfem::Operator / TimeDependentOperator surface ------------------------------------
    def Height(self) -> int:
        return int(self._lib.tpsrhs_height(self._h))

    def SetTime(self, t: float):
        self._time = float(t)

    def GetTime(self) -> float:
        return self._time

    def Mult(self, x: torch.Tensor, y: torch.Tensor, want_max_char_speed: bool = False):
        """``y = RHS(x)`` (``src/rhs_operator.cpp:343-464``).  Asynchronous on the operator's stream
        unless ``want_max_char_speed`` (the reference's ``max_char_speed`` side effect)."""
        self._check(x)
        self._check(y)
        mcs = C.c_double(0.0)
        st = self._lib.tpsrhs_mult(self._h, C.c_void_p(x.data_ptr()), C.c_void_p(y.data_ptr()), self._time,
                                   C.byref(mcs) if want_max_char_speed else None)
        if st != 0:
            raise TpsRhsError(st, "tpsrhs_mult")
        if want_max_char_speed:
            self.max_char_speed = mcs.value

    def updateGradients(self, x: torch.Tensor):
        self._check(x)
        st = self._lib.tpsrhs_update_gradients(self._h, C.c_void_p(x.data_ptr()))
        if st != 0:
            raise TpsRhsError(st, "tpsrhs_update_gradients")

    def getPrimitives(self) -> torch.Tensor:
        out = torch.empty(self.num_equation * self.NDofs, dtype=torch.float64, device=self.device)
        st = self._lib.tpsrhs_get_primitives(self._h, C.c_void_p(out.data_ptr()))
        if st != 0:
            raise TpsRhsError(st, "tpsrhs_get_primitives")
        return out.view(self.num_equation, self.NDofs)

    def getGradients(self) -> torch.Tensor:
        out = torch.empty(self.dim * self.num_equation * self.NDofs, dtype=torch.float64, device=self.device)
        st = self._lib.tpsrhs_get_gradients(self._h, C.c_void_p(out.data_ptr()))
        if st != 0:
            raise TpsRhsError(st, "tpsrhs_get_gradients")
        return out.view(self.dim, self.num_equation, self.NDofs)

    def getFlux(self, x: torch.Tensor, part: str = "total", gradients_current: bool = False) -> torch.Tensor:
        """The nodal flux tensor of ``RHSoperator::GetFlux`` (``src/rhs_operator.cpp:493-559``) at the state ``x``:
        ``[dim, num_equation, NDofs]``, the layout of :meth:`getGradients`.  ``part``: ``"convective"``
        (``ComputeConvectiveFluxes``), ``"viscous"`` (``ComputeViscousFluxes``, its sign) or ``"total"`` (their difference).
        ``Up`` and ``gradUp`` of the operator are refreshed from ``x`` first unless ``gradients_current`` (the caller has
        just run ``Mult(x)`` or ``updateGradients(x)``).  Asynchronous on the operator's stream."""
        self._check(x)
        out = torch.empty((self.dim, self.num_equation, self.NDofs), dtype=torch.float64, device=self.device)
        st = self._lib.tpsrhs_get_flux(self._h, C.c_void_p(x.data_ptr()), capi.flux_part(part), 1 if gradients_current else 0,
                                       C.c_void_p(out.data_ptr()))
        if st != 0:
            raise TpsRhsError(st, "tpsrhs_get_flux")
        return out

    def getPlasmaConductivity(self, x: torch.Tensor) -> torch.Tensor:
        """``plasma_conductivity_`` of ``SourceTerm`` (``src/source_term.cpp:125-199``): sigma at the nodes of the state
        ``x`` -- what the EM solver of the coupled torch runs reads (mixtures and the table gas)."""
        self._check(x)
        out = torch.empty(self.NDofs, dtype=torch.float64, device=self.device)
        st = self._lib.tpsrhs_get_plasma_conductivity(self._h, C.c_void_p(x.data_ptr()), C.c_void_p(out.data_ptr()))
        if st != 0:
            raise TpsRhsError(st, "tpsrhs_get_plasma_conductivity")
        return out

    def visualizationLayout(self) -> "capi.VisLayout":
        """Rows of :meth:`visualizationFields` for this operator's physics (``tpsrhs_visualization_layout``, host only)."""
        return capi.visualization_layout(self._physics, self.dim, bool(self._disc.axisymmetric))

    def visualizationFields(self, x: torch.Tensor, species_names=None, return_array: bool = False):
        """The derived fields of ``M2ulPhyS::updateVisualizationVariables`` (``src/M2ulPhyS.cpp:4156-4263``) at the nodes of
        the state ``x``: an ordered dict from the reference's field name to a view of ONE ``[nrows, NDofs]`` device tensor
        (``[NDofs]`` per scalar field, ``[nvel, NDofs]`` for ``diff_vel_<sp>``).  ``Up`` and ``gradUp`` of the operator are
        refreshed from ``x`` first.  Asynchronous on the operator's stream.  ``return_array``: ``(dict, the whole tensor)``
        -- any rows of it go through :meth:`integrate`, :meth:`nodalStats` and :meth:`PointSampler.sample` as they are."""
        self._check(x)
        lay = self.visualizationLayout()
        names = capi.visualization_names(lay, species_names)
        out = torch.empty((lay.nrows, self.NDofs), dtype=torch.float64, device=self.device)
        st = self._lib.tpsrhs_visualization_fields(self._h, C.c_void_p(x.data_ptr()), C.c_void_p(out.data_ptr()))
        if st != 0:
            raise TpsRhsError(st, "tpsrhs_visualization_fields")
        fields = {name: (out[first] if rows == 1 else out[first:first + rows]) for name, first, rows in names}
        return (fields, out) if return_array else fields

    # -- measurement helpers -----------------------------------------------------------------
    def enable_kernel_timing(self, on=True):
        self._lib.tpsrhs_enable_kernel_timing(self._h, 1 if on else 0)

    def kernel_times(self):
        names = (C.c_char_p * 8)()
        ms = (C.c_double * 8)()
        n = self._lib.tpsrhs_kernel_times(self._h, 8, names, ms)
        return {names[i].decode(): ms[i] for i in range(n)}

    def mult_times(self):
        """Device milliseconds of each ``Mult`` since timing was enabled (at most the last 128)."""
        ms = (C.c_double * 128)()
        n = self._lib.tpsrhs_mult_times(self._h, 128, ms)
        return [ms[i] for i in range(n)]

    def rk4_step(self, x: torch.Tensor, time: float, dt: float, want_max_char_speed=False, want_nan_count=False):
        """One explicit RK4 step, ``x`` updated in place; returns the new time (the role of
        ``timeIntegrator->Step(*U, time, dt); Check_NAN(); Check_Undershoot();`` in
        ``M2ulPhyS::solveStep``, ``src/M2ulPhyS.cpp:2004-2008``)."""
        self._check(x)
        t = C.c_double(time)
        speed = C.c_double(0.0)
        bad = C.c_int64(0)
        st = self._lib.tpsrhs_rk4_step(self._h, C.c_void_p(x.data_ptr()), C.byref(t), float(dt),
                                       C.byref(speed) if want_max_char_speed else None,
                                       C.byref(bad) if want_nan_count else None)
        if st != 0:
            raise RuntimeError(f"tpsrhs_rk4_step: {capi.STATUS.get(st, st)}: {self._lib.tpsrhs_last_error().decode()}")
        if want_max_char_speed:
            self.max_char_speed = speed.value
        if want_nan_count:
            self.nan_count = bad.value
        return t.value

    def step(self, x: torch.Tensor, time: float, dt: float, integrator, want_max_char_speed=False, want_nan_count=False):
        """``rk4_step`` for any of the reference's integrators that are built (``time/integrator``,
        ``src/M2ulPhyS.cpp:721-739, 2722-2736``): ``integrator`` is the enum value (``capi.FORWARD_EULER`` ...) or the
        input string ``forwardEuler``, ``rk2``, ``rk3``, ``rk4``; ``rk6`` raises (UNSUPPORTED)."""
        self._check(x)
        t = C.c_double(time)
        speed = C.c_double(0.0)
        bad = C.c_int64(0)
        st = self._lib.tpsrhs_step(self._h, capi.integrator_value(integrator), C.c_void_p(x.data_ptr()), C.byref(t), float(dt),
                                   C.byref(speed) if want_max_char_speed else None,
                                   C.byref(bad) if want_nan_count else None)
        if st != 0:
            raise TpsRhsError(st, "tpsrhs_step")
        if want_max_char_speed:
            self.max_char_speed = speed.value
        if want_nan_count:
            self.nan_count = bad.value
        return t.value

    def advance(self, x: torch.Tensor, time: float, dt: float, num_steps: int, constant_dt=True, cfl=0.0, hmin=0.0,
                integrator="rk4"):
        """``num_steps`` times ``M2ulPhyS::solveStep`` (``src/M2ulPhyS.cpp:2004-2019``) with dt, time and the NaN
        census on the device; returns ``(time, next dt, NaN count)`` after ONE synchronisation at the end.
        ``integrator``: as in :meth:`step`; the default is ``tpsrhs_advance`` itself."""
        self._check(x)
        t, d, bad = C.c_double(time), C.c_double(dt), C.c_int64(0)
        which = capi.integrator_value(integrator)
        if which == capi.RK4:
            st = self._lib.tpsrhs_advance(self._h, C.c_void_p(x.data_ptr()), C.byref(t), C.byref(d), int(num_steps),
                                          1 if constant_dt else 0, float(cfl), float(hmin), C.byref(bad))
            if st != 0:
                raise TpsRhsError(st, "tpsrhs_advance")
        else:
            st = self._lib.tpsrhs_advance_with(self._h, which, C.c_void_p(x.data_ptr()), C.byref(t), C.byref(d), int(num_steps),
                                               1 if constant_dt else 0, float(cfl), float(hmin), C.byref(bad))
            if st != 0:
                raise TpsRhsError(st, "tpsrhs_advance_with")
        return t.value, d.value, bad.value

    # -- running statistics (the reference's Averaging) ------------------------------------------------------------------
    def configureStatistics(self, sample_interval: int, start_iter: int = 0, variances: bool = True, iter0: int = 0):
        """``Averaging`` inside :meth:`advance` (``src/averaging.cpp:198-234, 331-435``): after every step of ``advance``
        the step counter goes up by one, and when it is a multiple of ``sample_interval`` (``sampleFreq``) and at least
        ``start_iter`` (``startIter``) the new state enters the running mean of the primitives (pressure in the
        temperature row) and, with ``variances``, the running velocity covariances.  ``iter0``: the step counter the
        loop continues from.  ``sample_interval = 0`` switches statistics off and frees the fields."""
        st = self._lib.tpsrhs_stats_configure(self._h, int(sample_interval), int(start_iter), 1 if variances else 0)
        if st != 0:
            raise TpsRhsError(st, "tpsrhs_stats_configure")
        if sample_interval != 0:
            st = self._lib.tpsrhs_stats_set_iter(self._h, int(iter0))
            if st != 0:
                raise TpsRhsError(st, "tpsrhs_stats_set_iter")

    def addSample(self, x: torch.Tensor):
        """One unconditional sample of ``x`` (``Averaging::addSample`` for a caller that drives the loop itself);
        asynchronous on the operator's stream."""
        self._check(x)
        st = self._lib.tpsrhs_stats_add_sample(self._h, C.c_void_p(x.data_ptr()))
        if st != 0:
            raise TpsRhsError(st, "tpsrhs_stats_add_sample")

    def numVariances(self) -> int:
        n = C.c_int(0)
        st = self._lib.tpsrhs_stats_num_variances(self._h, C.byref(n))
        if st != 0:
            raise TpsRhsError(st, "tpsrhs_stats_num_variances")
        return n.value

    def getStatistics(self):
        """``(mean, vari, ns_mean, ns_vari, iter)``: ``mean`` (num_equation, NDofs) and ``vari`` (nvar, NDofs; ``None``
        when only the mean is kept) as new CUDA tensors -- the reference's ``meanUp`` and ``rms`` -- and its
        ``samplesMean``, ``samplesRMS`` and ``iter``."""
        nvar = self.numVariances()
        mean = torch.empty(self.num_equation * self.NDofs, dtype=torch.float64, device=self.device)
        vari = torch.empty(nvar * self.NDofs, dtype=torch.float64, device=self.device) if nvar else None
        nm, nv, it = C.c_int(0), C.c_int(0), C.c_int64(0)
        st = self._lib.tpsrhs_stats_get(self._h, C.c_void_p(mean.data_ptr()), C.c_void_p(vari.data_ptr()) if nvar else None,
                                        C.byref(nm), C.byref(nv), C.byref(it))
        if st != 0:
            raise TpsRhsError(st, "tpsrhs_stats_get")
        return (mean.view(self.num_equation, self.NDofs), vari.view(nvar, self.NDofs) if nvar else None, nm.value, nv.value,
                it.value)

    def setStatistics(self, mean, vari, ns_mean: int, ns_vari: int = 0, iter0=None):
        """Continuation (``enableContinuation``): the fields and counters of an earlier run.  ``vari=None`` or
        ``ns_vari=0`` is ``restartRMS``: the covariances start again and the mean goes on."""
        for t, rows in ((mean, self.num_equation), (vari, None)):
            if t is None:
                continue
            rows = self.numVariances() if rows is None else rows
            if t.dtype != torch.float64 or not t.is_cuda or not t.is_contiguous() or t.numel() != rows * self.NDofs:
                raise ValueError(f"expected a contiguous float64 CUDA tensor of {rows} * NDofs entries")
        st = self._lib.tpsrhs_stats_set(self._h, C.c_void_p(mean.data_ptr()) if mean is not None else None,
                                        C.c_void_p(vari.data_ptr()) if vari is not None else None, int(ns_mean), int(ns_vari))
        if st != 0:
            raise TpsRhsError(st, "tpsrhs_stats_set")
        if iter0 is not None:
            st = self._lib.tpsrhs_stats_set_iter(self._h, int(iter0))
            if st != 0:
                raise TpsRhsError(st, "tpsrhs_stats_set_iter")

    # -- fields at arbitrary points: planes and probes ----------------------------------------------------------------------
    def createSampler(self, xyz, tol: float = 0.0, fill: float = 0.0) -> "PointSampler":
        """``FindPointsGSLIB::Setup`` + ``FindPoints`` on this operator's mesh (``src/gslib_interpolator.cpp:53-67``):
        ``xyz`` is a host array ``(dim, npts)``; ``tol <= 0`` is 1e-10; ``fill`` is the value of points outside the mesh.
        A float64 CUDA tensor ``(dim, npts)`` takes the device route instead (``tpsrhs_sampler_create_device``): the points
        are located by a kernel, keep their order and never visit the host -- meant for point sets that are spatially
        coherent already, such as :meth:`nodeCoordinates` of another operator.
        The operator owns the sampler: closing the operator closes it."""
        s = PointSampler(self, xyz, tol, fill)
        self._samplers = [w for w in getattr(self, "_samplers", []) if w() is not None] + [weakref.ref(s)]
        return s

    def nodeCoordinates(self) -> torch.Tensor:
        """Physical coordinates of the DG nodes, a new CUDA tensor ``(dim, NDofs)`` (``tpsrhs_node_coordinates``): what
        ``utils/pfield_interpolate.cpp:114-135`` forms with ``ElementTransformation::Transform``; the device counterpart
        of :func:`node_coordinates`.  Asynchronous on the operator's stream."""
        out = torch.empty((self.dim, self.NDofs), dtype=torch.float64, device=self.device)
        st = self._lib.tpsrhs_node_coordinates(self._h, C.c_void_p(out.data_ptr()))
        if st != 0:
            raise TpsRhsError(st, "tpsrhs_node_coordinates")
        return out

    # -- fields on a refined element lattice: what a ParaView output step evaluates ---------------------------------------
    def latticeSize(self, levels: int):
        """``(points_per_element, npts)`` of the closed uniform lattice with ``levels`` intervals per direction
        (``tpsrhs_lattice_size``): ``(levels + 1)^dim`` and that times the element count.  Host only."""
        ppe, npts = C.c_int64(0), C.c_int64(0)
        st = self._lib.tpsrhs_lattice_size(self._h, int(levels), C.byref(ppe), C.byref(npts))
        if st != 0:
            raise TpsRhsError(st, "tpsrhs_lattice_size")
        return ppe.value, npts.value

    def latticeCoordinates(self, levels: int) -> torch.Tensor:
        """Physical coordinates of the lattice points, a new CUDA tensor ``(dim, npts)`` (``tpsrhs_lattice_coordinates``);
        point ``e * (levels + 1)^dim + a + b (levels + 1) + c (levels + 1)^2``.  A corner is the element's vertex bit for
        bit.  Asynchronous on the operator's stream."""
        _, npts = self.latticeSize(levels)
        out = torch.empty((self.dim, npts), dtype=torch.float64, device=self.device)
        st = self._lib.tpsrhs_lattice_coordinates(self._h, int(levels), C.c_void_p(out.data_ptr()))
        if st != 0:
            raise TpsRhsError(st, "tpsrhs_lattice_coordinates")
        return out

    def latticeFields(self, field: torch.Tensor, levels: int, dtype=torch.float64) -> torch.Tensor:
        """``field`` (a float64 CUDA tensor of ``nrows * NDofs`` entries, byNODES: ``[NDofs]`` or ``[nrows, NDofs]``) at the
        lattice points of every element, each element with its own polynomial (``tpsrhs_lattice_fields``): a new CUDA
        tensor ``(nrows, npts)`` of ``dtype`` float64, or float32 -- the double value rounded once.  Asynchronous on the
        operator's stream."""
        if dtype not in (torch.float64, torch.float32):
            raise ValueError("dtype is torch.float64 or torch.float32")
        nrows = self._rows(field)
        _, npts = self.latticeSize(levels)
        out = torch.empty((nrows, npts), dtype=dtype, device=field.device)
        st = self._lib.tpsrhs_lattice_fields(self._h, int(levels), nrows, C.c_void_p(field.data_ptr()),
                                             C.c_void_p(out.data_ptr()), 1 if dtype == torch.float32 else 0)
        if st != 0:
            raise TpsRhsError(st, "tpsrhs_lattice_fields")
        return out

    def transferFrom(self, src_op: "RHSoperator", field: torch.Tensor, tol: float = 0.0, fill: float = 0.0):
        """``field`` of ``src_op`` at the nodes of this operator (``tpsrhs_transfer``; ``utils/pfield_interpolate.cpp:138-146``
        and ``CycleAvgJouleCoupling``): ``field`` is a float64 CUDA tensor of ``nrows * src_op.NDofs`` entries (byNODES);
        returns ``(tensor (nrows, NDofs), num_missing)``.  Nodes outside the mesh of ``src_op`` get ``fill`` in every row
        and are counted.  The first call for a pair of operators locates the nodes on the device and keeps the result on
        ``src_op``; later calls only evaluate.  Meshes, orders and bases may differ; the dimension may not."""
        if not isinstance(src_op, RHSoperator) or not getattr(src_op, "_h", None) or not getattr(self, "_h", None):
            raise ValueError("expected a live RHSoperator as the source")
        nrows = src_op._rows(field)
        out = torch.empty((nrows, self.NDofs), dtype=torch.float64, device=field.device)
        missing = C.c_int64(0)
        st = self._lib.tpsrhs_transfer(src_op._h, self._h, nrows, C.c_void_p(field.data_ptr()), C.c_void_p(out.data_ptr()),
                                       float(tol), float(fill), C.byref(missing))
        if st != 0:
            raise TpsRhsError(st, "tpsrhs_transfer")
        return out, missing.value

    def transferStats(self):
        """``(located, cache hits)`` of the ``tpsrhs_transfer`` calls with this operator as the source: how many located
        the target's nodes (ran ``k_locate``) and how many found a sampler from an earlier call."""
        a, b = C.c_int64(0), C.c_int64(0)
        st = self._lib.tpsrhs_transfer_stats(self._h, C.byref(a), C.byref(b))
        if st != 0:
            raise TpsRhsError(st, "tpsrhs_transfer_stats")
        return a.value, b.value

    def configureProbes(self, sampler, interval: int, capacity: int):
        """Probe records inside :meth:`advance`: after every step a counter goes up (zeroed here), and when it is a
        multiple of ``interval`` the conserved state at the sampler's points, the device-side time and the count are
        appended to a device buffer of ``capacity`` records; further records are dropped and counted.
        ``sampler=None`` or ``interval=0`` switches the probes off."""
        st = self._lib.tpsrhs_probe_configure(self._h, sampler._s if sampler is not None else None, int(interval), int(capacity))
        if st != 0:
            raise TpsRhsError(st, "tpsrhs_probe_configure")
        self._probe = (sampler, int(capacity)) if sampler is not None and interval != 0 else None

    def readProbes(self, reset: bool = False):
        """``(iters (nrec,), times (nrec,), values (nrec, num_equation, npts), ndropped)`` as numpy arrays; synchronises.
        ``reset`` starts the buffer again and leaves the step counter alone."""
        if getattr(self, "_probe", None) is None:
            raise TpsRhsError(self._lib.tpsrhs_probe_read(self._h, None, None, None, None, None, 0), "tpsrhs_probe_read")
        sampler, capacity = self._probe
        iters = np.zeros(capacity, dtype=np.int64)
        times = np.zeros(capacity)
        values = np.zeros((capacity, self.num_equation, sampler.npts))
        nrec, ndrop = C.c_int64(0), C.c_int64(0)
        st = self._lib.tpsrhs_probe_read(self._h, C.byref(nrec), C.byref(ndrop), iters.ctypes.data, times.ctypes.data,
                                         values.ctypes.data, 1 if reset else 0)
        if st != 0:
            raise TpsRhsError(st, "tpsrhs_probe_read")
        n = nrec.value
        return iters[:n].copy(), times[:n].copy(), values[:n].copy(), ndrop.value

    def setDt(self, dt: float):
        """The ``dt`` the non-reflecting boundary conditions advance their boundary state with in every
        ``Mult`` (the reference's ``BoundaryCondition::dt`` is a reference to ``M2ulPhyS::dt``)."""
        st = self._lib.tpsrhs_set_dt(self._h, float(dt))
        if st != 0:
            raise TpsRhsError(st, "tpsrhs_set_dt")

    def setForcing(self, forcing):
        """ConstantPressureGradient / SpongeZone / HeatSource of the reference's ``forcing`` array
        (``src/rhs_operator.cpp:101-123``); ``forcing``: :class:`tps_amd.capi.Forcing` or ``None``."""
        st = self._lib.tpsrhs_set_forcing(self._h, C.byref(forcing) if forcing is not None else None)
        if st != 0:
            raise TpsRhsError(st, "tpsrhs_set_forcing")

    def setJouleHeating(self, joule_heating):
        """The ``joule_heating_`` grid function of ``JouleHeating`` (``src/forcing_terms.cpp:443-471``): a
        float64 CUDA tensor of NDofs entries the operator reads at every ``Mult`` (kept alive here), or ``None``."""
        if joule_heating is not None:
            if (joule_heating.dtype != torch.float64 or not joule_heating.is_cuda or not joule_heating.is_contiguous()
                    or joule_heating.numel() != self.NDofs):
                raise ValueError("expected a contiguous float64 CUDA tensor of NDofs entries")
        self._joule = joule_heating
        st = self._lib.tpsrhs_set_joule_heating(
            self._h, C.c_void_p(joule_heating.data_ptr()) if joule_heating is not None else None)
        if st != 0:
            raise TpsRhsError(st, "tpsrhs_set_joule_heating")

    def setReactionRates(self, rates):
        """``M2ulPhyS::fetch`` (``src/M2ulPhyS2Boltzmann.cpp:89-101``): the forward rate coefficients of the reactions with
        ``model = bte`` (``capi.GRIDFUNCTION_RXN``), a float64 CUDA tensor ``[num_components, NDofs]`` the operator reads at
        every ``Mult`` (kept alive here; component = the reaction's ``bte/index``), or ``None``: those reactions then have
        ``k_f = 0``.  The shape is checked by the library (``TPSRHS_ERR_INVALID_ARGUMENT``)."""
        if rates is not None:
            if rates.dtype != torch.float64 or not rates.is_cuda or not rates.is_contiguous() or rates.dim() != 2:
                raise ValueError("expected a contiguous float64 CUDA tensor [num_components, NDofs]")
        st = self._lib.tpsrhs_set_reaction_rates(
            self._h, C.c_void_p(rates.data_ptr()) if rates is not None else None,
            int(rates.shape[0]) if rates is not None else 0, int(rates.shape[1]) if rates is not None else 0)
        if st != 0:
            raise TpsRhsError(st, "tpsrhs_set_reaction_rates")
        self._reaction_rates = rates

    def boltzmannFields(self, x: torch.Tensor, num_species=None) -> torch.Tensor:
        """``M2ulPhyS::push`` (``src/M2ulPhyS2Boltzmann.cpp:40-87``): a ``[num_species + 2, NDofs]`` device tensor -- the
        number densities of the first ``num_species`` species in particles per m^3 (default: all of them), then the heavy and
        the electron temperature -- at the nodes of the state ``x``.  Asynchronous on the operator's stream."""
        self._check(x)
        nsp = int(self._physics.mixture.num_species) if num_species is None else int(num_species)
        out = torch.empty((max(nsp, 0) + 2, self.NDofs), dtype=torch.float64, device=self.device)
        st = self._lib.tpsrhs_boltzmann_fields(self._h, C.c_void_p(x.data_ptr()), nsp, C.c_void_p(out.data_ptr()))
        if st != 0:
            raise TpsRhsError(st, "tpsrhs_boltzmann_fields")
        return out

    def lteComposition(self, T: torch.Tensor, p: torch.Tensor) -> torch.Tensor:
        """``PerfectMixture::GetSpeciesFromLTE(T, p, n_sp)`` (``src/equation_of_state.cpp:2096-2187``): the equilibrium number
        densities ``[num_species, n]`` in mol/m^3 at the temperatures ``T`` [K] and pressures ``p`` [Pa] (float64 device
        tensors of ``n`` entries) -- Saha for the electrons, Boltzmann for the levels of the neutral.  Synchronous."""
        for t in (T, p):
            if t.dtype != torch.float64 or not t.is_cuda or not t.is_contiguous() or t.dim() != 1:
                raise ValueError("expected contiguous one-dimensional float64 CUDA tensors")
        if T.numel() != p.numel():
            raise ValueError("T and p must have the same number of entries")
        out = torch.empty((int(self._physics.mixture.num_species), T.numel()), dtype=torch.float64, device=self.device)
        st = self._lib.tpsrhs_lte_composition(self._h, T.numel(), C.c_void_p(T.data_ptr()), C.c_void_p(p.data_ptr()),
                                              C.c_void_p(out.data_ptr()))
        if st != 0:
            raise TpsRhsError(st, "tpsrhs_lte_composition")
        return out

    def speciesFromLTE(self, x: torch.Tensor, tables, want_primitives: bool = False):
        """``M2ulPhyS::initilizeSpeciesFromLTE`` (``src/M2ulPhyS.cpp:2388-2461``, ``io/restartFromLTE = True``) and the species
        clamp of ``Check_Undershoot``: ``x`` (the operator's state vector) holds rho, rho u, rho E of an LTE solution in its
        rows ``0 .. nvel + 1``; every row is rewritten in place with the species state in equilibrium at the temperature and
        pressure of the table gas.  ``tables``: a ``capi.LteRestart`` (``capi.make_lte_restart``).  Returns the
        ``capi.LteRestartReport``, or ``(report, Up [num_equation, NDofs])`` with ``want_primitives``.  Synchronous."""
        self._check(x)
        up = torch.empty((self.num_equation, self.NDofs), dtype=torch.float64, device=self.device) if want_primitives else None
        rep = capi.LteRestartReport()
        st = self._lib.tpsrhs_species_from_lte(self._h, C.byref(tables), C.c_void_p(x.data_ptr()),
                                               C.c_void_p(up.data_ptr()) if up is not None else None, C.byref(rep))
        if st != 0:
            raise TpsRhsError(st, "tpsrhs_species_from_lte")
        return (rep, up) if want_primitives else rep

    def setMixingLength(self, distance, max_mixing_length=0.0, pr_ratio=1.0, lewis=1.0, bulk_multiplier=0.0):
        """``MixingLengthTransport`` (``src/mixing_length_transport.cpp``, ``[flow] useMixingLength``): ``distance`` =
        the wall-distance grid function, a float64 CUDA tensor of NDofs entries read at every ``Mult`` (kept alive
        here), or ``None`` to switch the model off."""
        if distance is not None:
            if (distance.dtype != torch.float64 or not distance.is_cuda or not distance.is_contiguous()
                    or distance.numel() != self.NDofs):
                raise ValueError("expected a contiguous float64 CUDA tensor of NDofs entries")
        self._distance = distance
        prm = capi.MixingLength(float(max_mixing_length), float(pr_ratio), float(lewis), float(bulk_multiplier))
        st = self._lib.tpsrhs_set_mixing_length(self._h, C.c_void_p(distance.data_ptr()) if distance is not None else None,
                                                C.byref(prm))
        if st != 0:
            raise TpsRhsError(st, "tpsrhs_set_mixing_length")

    def wallDistance(self, faces=None, attributes=None) -> torch.Tensor:
        """The wall-distance grid function ``distance_`` the reference fills at start-up when ``flow/computeDistance`` is set
        (``evaluateDistanceSerial``, ``src/utils.cpp:371-514``): the distance from every node to the nearest of ``faces``
        (``(nf, 2^(dim-1), dim)`` corner coordinates, :func:`tps_amd.capi.wall_faces`), a new float64 CUDA tensor of NDofs
        entries -- what :meth:`setMixingLength` takes.  ``faces=None``: the wall faces of the operator's own mesh, selected
        by ``attributes`` or, with ``attributes=None``, by its boundary conditions (every wall that is not inviscid).  On a
        partitioned mesh pass the concatenation of the wall faces of all ranks.  Without faces every entry is 1e30."""
        if faces is None:
            faces = capi.wall_faces(self._mesh, self._bc_list, attributes)
        faces = np.ascontiguousarray(faces, dtype=np.float64)
        if faces.size == 0:
            faces = faces.reshape(0, 1 << (self.dim - 1), self.dim)
        if faces.ndim != 3 or faces.shape[1:] != (1 << (self.dim - 1), self.dim):
            raise ValueError("expected the faces as an array (nf, 2^(dim-1), dim)")
        out = torch.empty(self.NDofs, dtype=torch.float64, device=self.device)
        st = self._lib.tpsrhs_wall_distance(self._h, int(faces.shape[0]), faces.ctypes.data if faces.size else None,
                                            C.c_void_p(out.data_ptr()))
        if st != 0:
            raise TpsRhsError(st, "tpsrhs_wall_distance")
        return out

    # -- volume integrals, extrema and the monitor history --------------------------------------------------------------------
    def _rows(self, field: torch.Tensor) -> int:
        n = self.NDofs
        if field.dtype != torch.float64 or not field.is_cuda or not field.is_contiguous() or field.numel() % n or not field.numel():
            raise ValueError("expected a contiguous float64 CUDA tensor of nrows * NDofs entries")
        return field.numel() // n

    def integrate(self, field: torch.Tensor, exact_q=None, radial=None):
        """``(sum, sumsq)``, each a new CUDA tensor ``(nrows,)``: ``sum_q W_q g_q`` and ``sum_q W_q g_q^2`` of
        ``g = field - exact_q`` on MFEM's default rule of ``GridFunction::ComputeLpError`` (Gauss-Legendre, order 2p + 3),
        so that ``sumsq.sqrt()`` is the L2 error ``M2ulPhyS::checkSolutionError`` prints (``src/masa_handler.cpp:139-152``).
        ``field``: ``nrows * NDofs`` entries (byNODES); ``exact_q``: ``(nrows, npts)`` at the points of
        :func:`quadrature_points`, or ``None`` for 0; ``radial``: weight every point by its first coordinate (``None``:
        the operator's axisymmetric flag).  Asynchronous on the operator's stream."""
        nrows = self._rows(field)
        if exact_q is not None:
            if (exact_q.dtype != torch.float64 or not exact_q.is_cuda or not exact_q.is_contiguous()
                    or exact_q.numel() != nrows * self.numQuadraturePoints()):
                raise ValueError("expected exact_q as a contiguous float64 CUDA tensor of nrows * npts entries")
        if radial is None:
            radial = bool(self._disc.axisymmetric)
        out = torch.empty((2, nrows), dtype=torch.float64, device=field.device)
        st = self._lib.tpsrhs_integrate(self._h, nrows, C.c_void_p(field.data_ptr()),
                                        C.c_void_p(exact_q.data_ptr()) if exact_q is not None else None, 1 if radial else 0,
                                        C.c_void_p(out[0].data_ptr()), C.c_void_p(out[1].data_ptr()))
        if st != 0:
            raise TpsRhsError(st, "tpsrhs_integrate")
        return out[0], out[1]

    def numQuadraturePoints(self) -> int:
        return self._mesh.num_elements * (self._disc.order + 2) ** self.dim

    def nodalStats(self, field: torch.Tensor):
        """``(min, max, meanabs)`` of every row of ``field`` (``nrows * NDofs`` entries), new CUDA tensors ``(nrows,)``;
        ``meanabs = sum |f| / NDofs`` is ``RHSoperator::computeMeanTimeDerivatives`` (``src/rhs_operator.cpp:833-849``)
        for ``field = Mult(x)``.  A NaN entry never wins min / max and does poison meanabs."""
        nrows = self._rows(field)
        out = torch.empty((3, nrows), dtype=torch.float64, device=field.device)
        st = self._lib.tpsrhs_nodal_stats(self._h, nrows, C.c_void_p(field.data_ptr()), C.c_void_p(out[0].data_ptr()),
                                          C.c_void_p(out[1].data_ptr()), C.c_void_p(out[2].data_ptr()))
        if st != 0:
            raise TpsRhsError(st, "tpsrhs_nodal_stats")
        return out[0], out[1], out[2]

    def configureMonitor(self, interval: int, capacity: int):
        """Monitor records inside :meth:`advance`: after every step a counter goes up (zeroed here), and when it is a
        multiple of ``interval`` the count, the device-side time, the ``dt`` of the next step, the integrals of the
        conserved state and its minima and maxima are appended to a device buffer of ``capacity`` records; further
        records are dropped and counted.  ``interval=0`` switches the monitor off."""
        st = self._lib.tpsrhs_monitor_configure(self._h, int(interval), int(capacity))
        if st != 0:
            raise TpsRhsError(st, "tpsrhs_monitor_configure")
        self._monitor = int(capacity) if interval != 0 else None

    def readMonitor(self, reset: bool = False):
        """``dict(iters (nrec,), times, dts (nrec,), totals, mins, maxs (nrec, num_equation), ndropped)`` as numpy arrays;
        synchronises.  ``reset`` starts the buffer again and leaves the step counter alone."""
        capacity = getattr(self, "_monitor", None)
        if capacity is None:
            raise TpsRhsError(self._lib.tpsrhs_monitor_read(self._h, None, None, None, None, None, None, None, None, 0),
                              "tpsrhs_monitor_read")
        iters = np.zeros(capacity, dtype=np.int64)
        times, dts = np.zeros(capacity), np.zeros(capacity)
        totals, mins, maxs = (np.zeros((capacity, self.num_equation)) for _ in range(3))
        nrec, ndrop = C.c_int64(0), C.c_int64(0)
        st = self._lib.tpsrhs_monitor_read(self._h, C.byref(nrec), C.byref(ndrop), iters.ctypes.data, times.ctypes.data,
                                           dts.ctypes.data, totals.ctypes.data, mins.ctypes.data, maxs.ctypes.data,
                                           1 if reset else 0)
        if st != 0:
            raise TpsRhsError(st, "tpsrhs_monitor_read")
        n = nrec.value
        return dict(iters=iters[:n].copy(), times=times[:n].copy(), dts=dts[:n].copy(), totals=totals[:n].copy(),
                    mins=mins[:n].copy(), maxs=maxs[:n].copy(), ndropped=ndrop.value)

    # -- the conservative positivity limiter (in place of Check_Undershoot's clamp, src/M2ulPhyS.cpp:2522-2548) --------------
    def limiterWeights(self) -> torch.Tensor:
        """``W_n = int_K l_n dV`` on the rule of :meth:`integrate` (with the radial factor when the operator is
        axisymmetric), a new CUDA tensor ``(NDofs,)``: ``(W * f).sum()`` is ``integrate(f)[0]`` up to rounding."""
        out = torch.empty(self.NDofs, dtype=torch.float64, device=self.device)
        st = self._lib.tpsrhs_limiter_weights(self._h, C.c_void_p(out.data_ptr()))
        if st != 0:
            raise TpsRhsError(st, "tpsrhs_limiter_weights")
        return out

    def limit(self, x: torch.Tensor, rows=None, floors=None, pressure_floor: float = 0.0):
        """One application of the Zhang-Shu linear scaling limiter to ``x`` in place, element by element: every listed
        row ends ``>= floor`` and every element mean stays where it was (``include/tpsrhs.h`` states the operation).
        ``rows=None``: the species rows ``Check_Undershoot`` clamps, floor 0; ``floors``: one number or one per row;
        ``pressure_floor > 0`` (dry air, row 0 listed with a floor > 0) adds the pressure step.  Asynchronous on the
        operator's stream; adds to the counters of :meth:`readLimiter`."""
        self._check(x)
        lim = capi.make_limiter(rows, floors, pressure_floor)
        st = self._lib.tpsrhs_limit(self._h, C.byref(lim), C.c_void_p(x.data_ptr()))
        if st != 0:
            raise TpsRhsError(st, "tpsrhs_limit")

    def configureLimiter(self, rows=None, floors=None, pressure_floor: float = 0.0, off: bool = False):
        """The limiter of the time loop: :meth:`step`, :meth:`rk4_step` and every step of :meth:`advance` end with one
        application (arguments as in :meth:`limit`), which takes the place of the species clamp on the rows it lists
        (all species rows or none).  The statistics, probes and monitor see the limited state.  ``off=True`` switches it
        off and the clamp is back."""
        lim = None if off else capi.make_limiter(rows, floors, pressure_floor)
        st = self._lib.tpsrhs_limiter_configure(self._h, C.byref(lim) if lim is not None else None)
        if st != 0:
            raise TpsRhsError(st, "tpsrhs_limiter_configure")

    def readLimiter(self, reset: bool = False):
        """``dict(calls, limited (num_equation,), clamped (num_equation,), pressure_limited, pressure_unfixable)``: the
        applications and the elements per outcome and state row since the last reset; synchronises."""
        rep = capi.LimiterReport()
        st = self._lib.tpsrhs_limiter_read(self._h, C.byref(rep), 1 if reset else 0)
        if st != 0:
            raise TpsRhsError(st, "tpsrhs_limiter_read")
        neq = self.num_equation
        return dict(calls=rep.calls, limited=np.array(rep.limited[:neq], dtype=np.int64),
                    clamped=np.array(rep.clamped[:neq], dtype=np.int64), pressure_limited=rep.pressure_limited,
                    pressure_unfixable=rep.pressure_unfixable)

    # -- Legendre modal filter and smoothness sensor -----------------------------------------------------------------------------
    def _check_rows(self, t: torch.Tensor, what: str):
        if not (t.is_cuda and t.dtype == torch.float64 and t.is_contiguous() and t.dim() in (1, 2) and t.shape[-1] == self.NDofs):
            raise ValueError(f"{what}: a contiguous float64 CUDA tensor (NDofs,) or (nrows, NDofs)")

    def modalTransform(self, field: torch.Tensor, inverse: bool = False) -> torch.Tensor:
        """The Legendre modal coefficients ``(V^-1 x ... x V^-1) u`` of every row of ``field`` ``(NDofs,)`` or
        ``(nrows, NDofs)``, element by element, in the node order of the element -- or, ``inverse=True``, the nodal values
        of such coefficients.  A new CUDA tensor of the same shape; asynchronous on the operator's stream."""
        self._check_rows(field, "modalTransform")
        out = torch.empty_like(field)
        nrows = 1 if field.dim() == 1 else field.shape[0]
        st = self._lib.tpsrhs_modal_transform(self._h, 1 if inverse else 0, nrows, C.c_void_p(field.data_ptr()),
                                              C.c_void_p(out.data_ptr()))
        if st != 0:
            raise TpsRhsError(st, "tpsrhs_modal_transform")
        return out

    def modalEnergy(self, field: torch.Tensor):
        """``(energy (ne, p + 1), sensor (ne,))`` of one scalar field ``(NDofs,)``: the reference-space L2 norm squared of
        every element split by the highest 1-D Legendre degree, and ``S = E_p / sum E`` (Persson & Peraire)."""
        self._check_rows(field, "modalEnergy")
        if field.dim() != 1:
            raise ValueError("modalEnergy: one scalar field (NDofs,)")
        ne = self.NDofs // (self._disc.order + 1) ** self.dim
        energy = torch.empty((ne, self._disc.order + 1), dtype=torch.float64, device=self.device)
        sensor = torch.empty(ne, dtype=torch.float64, device=self.device)
        st = self._lib.tpsrhs_modal_energy(self._h, C.c_void_p(field.data_ptr()), C.c_void_p(energy.data_ptr()),
                                           C.c_void_p(sensor.data_ptr()))
        if st != 0:
            raise TpsRhsError(st, "tpsrhs_modal_energy")
        return energy, sensor

    def modalFilter(self, x: torch.Tensor, **kw):
        """One application of the exponential modal filter to ``x`` in place (``include/tpsrhs.h`` states the operation);
        keywords as :func:`tps_amd.capi.make_modal_filter`: ``rows`` (default: every row), ``cutoff``, ``alpha``,
        ``exponent``, ``conservative``, ``sensor_row``, ``sensor_threshold``.  Asynchronous on the operator's stream; adds
        to the counters of :meth:`readModalFilter`."""
        self._check(x)
        f = capi.make_modal_filter(**kw)
        st = self._lib.tpsrhs_modal_filter_apply(self._h, C.byref(f), C.c_void_p(x.data_ptr()))
        if st != 0:
            raise TpsRhsError(st, "tpsrhs_modal_filter_apply")

    def configureModalFilter(self, off: bool = False, **kw):
        """The modal filter of the time loop: every step is the stage sequence, then one application of the filter
        (keywords as in :meth:`modalFilter`), then the limiter when one is configured.  The statistics, probes and
        monitor see the filtered state.  ``off=True`` switches it off."""
        f = None if off else capi.make_modal_filter(**kw)
        st = self._lib.tpsrhs_modal_filter_configure(self._h, C.byref(f) if f is not None else None)
        if st != 0:
            raise TpsRhsError(st, "tpsrhs_modal_filter_configure")

    def readModalFilter(self, reset: bool = False):
        """``dict(calls, elements_seen, elements_filtered)`` since the last reset; synchronises."""
        rep = capi.ModalFilterReport()
        st = self._lib.tpsrhs_modal_filter_read(self._h, C.byref(rep), 1 if reset else 0)
        if st != 0:
            raise TpsRhsError(st, "tpsrhs_modal_filter_read")
        return dict(calls=rep.calls, elements_seen=rep.elements_seen, elements_filtered=rep.elements_filtered)

    # -- surface integrals over boundary patches and their history -----------------------------------------------------------
    def createSurface(self, attributes=None, faces=None) -> "Surface":
        """A set of element faces in patches (``tpsrhs_surface_create``).  ``attributes``: the boundary attributes of the
        operator's mesh, one patch each (:func:`tps_amd.capi.patch_faces` -- the faces
        ``BoundaryCondition::aggregateBndryFaces`` counts, ``src/BoundaryCondition.cpp:76-92``).  ``faces``: an explicit
        ``(elem, face, patch)`` triple of integer arrays, ``face = 2 d + s``; any element face may be listed, also an
        interior one; the number of patches is ``max(patch) + 1``, or ``(elem, face, patch, num_patches)``.
        The operator owns the surface: closing the operator closes it."""
        if (attributes is None) == (faces is None):
            raise ValueError("give either the boundary attributes or the faces")
        if attributes is not None:
            attributes = np.ascontiguousarray(attributes, dtype=np.int32).ravel()
            elem, face, patch = capi.patch_faces(self._mesh, attributes)
            npatch = int(attributes.size)
        else:
            elem, face, patch = (np.ascontiguousarray(a, dtype=np.int32).ravel() for a in faces[:3])
            npatch = int(faces[3]) if len(faces) > 3 else (int(patch.max()) + 1 if patch.size else 1)
            if not (elem.size == face.size == patch.size):
                raise ValueError("elem, face and patch must have the same length")
        s = Surface(self, npatch, elem, face, patch)
        self._surfaces = [w for w in getattr(self, "_surfaces", []) if w() is not None] + [weakref.ref(s)]
        return s

    def surfaceMonitor(self, surface, interval: int, capacity: int):
        """Patch history inside :meth:`advance`: after every step a counter goes up (zeroed here), and when it is a
        multiple of ``interval`` the count, the device-side time, the integrals of the conserved state over every patch of
        ``surface`` and the mass flow through it are appended to a device buffer of ``capacity`` records; further records
        are dropped and counted.  ``surface=None`` or ``interval=0`` switches the history off."""
        st = self._lib.tpsrhs_surface_monitor_configure(self._h, surface._s if surface is not None else None, int(interval),
                                                        int(capacity))
        if st != 0:
            raise TpsRhsError(st, "tpsrhs_surface_monitor_configure")
        # (a weak reference: the operator does not keep the surface alive, and the two form no cycle)
        self._surface_monitor = ((weakref.ref(surface), surface.num_patches, int(capacity))
                                 if surface is not None and interval != 0 else None)

    def readSurfaceMonitor(self, reset: bool = False):
        """``dict(iters (nrec,), times (nrec,), integrals (nrec, npatch, num_equation), mass_flow (nrec, npatch), ndropped)``
        as numpy arrays; synchronises.  ``reset`` starts the buffer again and leaves the step counter alone."""
        if getattr(self, "_surface_monitor", None) is None:
            raise TpsRhsError(self._lib.tpsrhs_surface_monitor_read(self._h, None, None, None, None, None, None, 0),
                              "tpsrhs_surface_monitor_read")
        _, npatch, capacity = self._surface_monitor
        iters = np.zeros(capacity, dtype=np.int64)
        times = np.zeros(capacity)
        integrals = np.zeros((capacity, npatch, self.num_equation))
        mass_flow = np.zeros((capacity, npatch))
        nrec, ndrop = C.c_int64(0), C.c_int64(0)
        st = self._lib.tpsrhs_surface_monitor_read(self._h, C.byref(nrec), C.byref(ndrop), iters.ctypes.data, times.ctypes.data,
                                                   integrals.ctypes.data, mass_flow.ctypes.data, 1 if reset else 0)
        if st != 0:
            raise TpsRhsError(st, "tpsrhs_surface_monitor_read")
        n = nrec.value
        return dict(iters=iters[:n].copy(), times=times[:n].copy(), integrals=integrals[:n].copy(),
                    mass_flow=mass_flow[:n].copy(), ndropped=ndrop.value)

    def kernel_bytes(self):
        names = (C.c_char_p * 8)()
        b = (C.c_double * 8)()
        n = self._lib.tpsrhs_kernel_bytes(self._h, 8, names, b)
        return {names[i].decode(): b[i] for i in range(n)}

    def _check(self, t: torch.Tensor):
        if t.dtype != torch.float64 or not t.is_cuda or not t.is_contiguous() or t.numel() != self.Height():
            raise ValueError("expected a contiguous float64 CUDA tensor of num_equation*NDofs entries")

    def close(self):
        if getattr(self, "_h", None):
            for w in getattr(self, "_samplers", []):  # tpsrhs_destroy frees them: their handles die here
                if w() is not None:
                    w()._s = None
            for w in getattr(self, "_surfaces", []):
                if w() is not None:
                    w()._s = None
            self._probe = None
            self._surface_monitor = None
            self._lib.tpsrhs_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PointSampler:
    """A set of points located in one operator's mesh (``tpsrhs_sampler_*``): the reference's ``InterpolatorBase`` after
    ``initializeFinder`` and ``setInterpolationPoints`` (``src/gslib_interpolator.cpp:53-67``)."""

    def __init__(self, op: RHSoperator, xyz, tol: float = 0.0, fill: float = 0.0):
        self._lib = capi.load()
        self._op = op
        s = C.c_void_p()
        if isinstance(xyz, torch.Tensor) and xyz.is_cuda:  # located on the device, in the caller's order
            if xyz.dtype != torch.float64 or not xyz.is_contiguous() or xyz.dim() != 2 or xyz.shape[0] != op.dim:
                raise ValueError("expected the points as a contiguous float64 CUDA tensor (dim, npts)")
            self.npts = int(xyz.shape[1])
            st = self._lib.tpsrhs_sampler_create_device(op._h, self.npts, C.c_void_p(xyz.data_ptr()), float(tol), float(fill),
                                                        C.byref(s))
            if st != 0:
                raise TpsRhsError(st, "tpsrhs_sampler_create_device")
            self._xyz = xyz  # read on the operator's stream: alive at least as long as the sampler
            self._s = s
            return
        xyz = np.ascontiguousarray(xyz, dtype=np.float64)
        if xyz.ndim != 2 or xyz.shape[0] != op.dim:
            raise ValueError("expected the points as an array (dim, npts)")
        self.npts = int(xyz.shape[1])
        st = self._lib.tpsrhs_sampler_create(op._h, self.npts, xyz.ctypes.data, float(tol), float(fill), C.byref(s))
        if st != 0:
            raise TpsRhsError(st, "tpsrhs_sampler_create")
        self._s = s

    def info(self):
        """``(elem (npts,), ref (dim, npts), nfound)``: the element of every point (-1: not found) and its reference
        coordinates in [0,1], in the caller's order."""
        elem = np.zeros(self.npts, dtype=np.int32)
        ref = np.zeros((self._op.dim, self.npts))
        n, nf = C.c_int64(0), C.c_int64(0)
        st = self._lib.tpsrhs_sampler_info(self._s, C.byref(n), C.byref(nf), elem.ctypes.data, ref.ctypes.data)
        if st != 0:
            raise TpsRhsError(st, "tpsrhs_sampler_info")
        return elem, ref, nf.value

    def sample(self, field: torch.Tensor) -> torch.Tensor:
        """``FindPointsGSLIB::Interpolate`` (``src/gslib_interpolator.cpp:69-84``): ``field`` is a float64 CUDA tensor of
        ``nrows * NDofs`` entries (byNODES); returns ``(nrows, npts)``.  Asynchronous on the operator's stream."""
        n = self._op.NDofs
        if field.dtype != torch.float64 or not field.is_cuda or not field.is_contiguous() or field.numel() % n or not field.numel():
            raise ValueError("expected a contiguous float64 CUDA tensor of nrows * NDofs entries")
        nrows = field.numel() // n
        out = torch.empty((nrows, self.npts), dtype=torch.float64, device=field.device)
        if self.npts == 0:
            return out
        st = self._lib.tpsrhs_sample(self._s, nrows, C.c_void_p(field.data_ptr()), C.c_void_p(out.data_ptr()))
        if st != 0:
            raise TpsRhsError(st, "tpsrhs_sample")
        return out

    def close(self):
        if getattr(self, "_s", None):
            if getattr(self._op, "_probe", None) is not None and self._op._probe[0] is self:
                self._op._probe = None
            self._lib.tpsrhs_sampler_destroy(self._s)
        self._s = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Surface:
    """A set of element faces in patches on one operator's mesh (``tpsrhs_surface_*``): what the reference aggregates per
    inlet and outlet at start-up (``BoundaryCondition::aggregateArea`` / ``aggregateBndryFaces``,
    ``src/BoundaryCondition.cpp:59-92``), with the integrals of any byNODES array over it."""

    _FORMS = {"scalar": capi.SURFACE_SCALAR, "flux": capi.SURFACE_FLUX, "normal": capi.SURFACE_NORMAL}

    def __init__(self, op: RHSoperator, num_patches: int, elem, face, patch):
        self._lib = capi.load()
        self._op = op
        self.num_patches = int(num_patches)
        s = C.c_void_p()
        n = int(elem.size)
        st = self._lib.tpsrhs_surface_create(op._h, self.num_patches, n, elem.ctypes.data if n else None,
                                             face.ctypes.data if n else None, patch.ctypes.data if n else None, C.byref(s))
        if st != 0:
            raise TpsRhsError(st, "tpsrhs_surface_create")
        self._s = s

    def info(self):
        """``(num_patches, num_faces, faces_per_patch (num_patches,))``."""
        np_, nf = C.c_int(0), C.c_int64(0)
        per = np.zeros(self.num_patches, dtype=np.int64)
        st = self._lib.tpsrhs_surface_info(self._s, C.byref(np_), C.byref(nf), per.ctypes.data)
        if st != 0:
            raise TpsRhsError(st, "tpsrhs_surface_info")
        return np_.value, nf.value, per

    def integrate(self, field: torch.Tensor, form: str = "scalar", radial=None, row_stride=None, comp_stride=None) -> torch.Tensor:
        """The integrals of ``field`` over every patch, a new CUDA tensor: ``"scalar"`` -> ``(npatch, nrows)`` of
        ``int f dS``; ``"flux"`` -> ``(npatch, nrows)`` of ``int F . n dS``; ``"normal"`` -> ``(npatch, nrows, dim)`` of
        ``int f n dS``.  The value (row r, component c, node) is ``field.flatten()[r*row_stride + c*comp_stride + node]``.
        Defaults: ``row_stride = NDofs`` for scalar and normal; for flux ``field`` is ``[nrows][dim][NDofs]``
        (``row_stride = dim*NDofs``, ``comp_stride = NDofs``).  With explicit strides the number of rows is what fits into
        ``field``.  ``radial``: weight every point by its first coordinate (``None``: the operator's axisymmetric flag).
        Asynchronous on the operator's stream."""
        op = self._op
        if form not in self._FORMS:
            raise ValueError("form is one of 'scalar', 'flux', 'normal'")
        if field.dtype != torch.float64 or not field.is_cuda or not field.is_contiguous() or not field.numel():
            raise ValueError("expected a contiguous float64 CUDA tensor")
        n, dim = op.NDofs, op.dim
        ncomp = dim if form == "flux" else 1
        if comp_stride is None:
            comp_stride = n
        if row_stride is None:
            row_stride = ncomp * n
        # the rows whose last value still lies inside the field
        span = (ncomp - 1) * int(comp_stride) + n
        if field.numel() < span:
            raise ValueError("the field is shorter than one row")
        nrows = (field.numel() - span) // int(row_stride) + 1 if row_stride > 0 else 1
        if radial is None:
            radial = bool(op._disc.axisymmetric)
        shape = (self.num_patches, nrows, dim) if form == "normal" else (self.num_patches, nrows)
        out = torch.empty(shape, dtype=torch.float64, device=field.device)
        st = self._lib.tpsrhs_surface_integrate(self._s, self._FORMS[form], nrows, C.c_void_p(field.data_ptr()), int(row_stride),
                                                int(comp_stride), 1 if radial else 0, C.c_void_p(out.data_ptr()))
        if st != 0:
            raise TpsRhsError(st, "tpsrhs_surface_integrate")
        return out

    def loads(self, x: torch.Tensor, part: str = "total", gradients_current: bool = False) -> torch.Tensor:
        """``(npatch, num_equation)``: ``int F_part . n dS`` per patch of the nodal flux tensor of the state ``x``
        (:meth:`RHSoperator.getFlux` followed by the flux reduction, ``tpsrhs_surface_loads``).  ``n`` points out of the
        element: on a wall patch the momentum rows of ``"total"`` are the force the fluid exerts on the wall, the energy row
        the power leaving the fluid.  The flux is that of the interior trace, not the numerical boundary flux."""
        op = self._op
        op._check(x)
        out = torch.empty((self.num_patches, op.num_equation), dtype=torch.float64, device=op.device)
        st = self._lib.tpsrhs_surface_loads(self._s, C.c_void_p(x.data_ptr()), capi.flux_part(part), 1 if gradients_current else 0,
                                            C.c_void_p(out.data_ptr()))
        if st != 0:
            raise TpsRhsError(st, "tpsrhs_surface_loads")
        return out

    def area(self, radial=None) -> torch.Tensor:
        """``(npatch,)``: the scalar integral of ones -- ``BoundaryCondition::aggregateArea``
        (``src/BoundaryCondition.cpp:59-74``), the ``data[7]`` of the mass-flow outlets."""
        ones = torch.ones(self._op.NDofs, dtype=torch.float64, device=self._op.device)
        return self.integrate(ones, "scalar", radial=radial)[:, 0]

    def close(self):
        if getattr(self, "_s", None):
            if getattr(self._op, "_surface_monitor", None) is not None and self._op._surface_monitor[0]() is self:
                self._op._surface_monitor = None
            self._lib.tpsrhs_surface_destroy(self._s)
        self._s = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def locate_points(host_mesh, xyz, tol: float = 0.0):
    """Host-only call of ``tpsrhs_locate_points``: ``xyz`` ``(dim, npts)`` -> ``(elem (npts,), ref (dim, npts))``."""
    lib = capi.load()
    ma = capi.MeshArgs(host_mesh)
    xyz = np.ascontiguousarray(xyz, dtype=np.float64)
    if xyz.ndim != 2 or xyz.shape[0] != host_mesh.dim:
        raise ValueError("expected the points as an array (dim, npts)")
    npts = xyz.shape[1]
    elem = np.zeros(npts, dtype=np.int32)
    ref = np.zeros((host_mesh.dim, npts))
    st = lib.tpsrhs_locate_points(C.byref(ma.c), npts, xyz.ctypes.data, float(tol), elem.ctypes.data, ref.ctypes.data)
    if st != 0:
        raise TpsRhsError(st, "tpsrhs_locate_points")
    return elem, ref


def plane_points(point, normal, bb0, bb1, n: int) -> np.ndarray:
    """``PlaneInterpolator::setInterpolationPoints`` (``src/gslib_interpolator.cpp:121-190``): the ``(3, n*n)`` points of
    the plane through ``point`` with ``normal`` over the bounding box ``[bb0, bb1]``."""
    lib = capi.load()
    a = [(C.c_double * 3)(*[float(v) for v in w]) for w in (point, normal, bb0, bb1)]
    out = np.zeros((3, max(int(n), 0) ** 2))
    st = lib.tpsrhs_plane_points(a[0], a[1], a[2], a[3], int(n), out.ctypes.data)
    if st != 0:
        raise TpsRhsError(st, "tpsrhs_plane_points")
    return out


def quadrature_points(host_mesh, order: int):
    """Host-only call of ``tpsrhs_quadrature_points``: ``(xyz (dim, npts), w (npts,))``, the points and weights (without
    the radial factor) of the rule of :meth:`RHSoperator.integrate` -- tensor Gauss-Legendre with ``order + 2`` points per
    direction, point ``q = e * NQ^dim + (i + j NQ + k NQ^2)``."""
    lib = capi.load()
    ma = capi.MeshArgs(host_mesh)
    n = C.c_int64(0)
    st = lib.tpsrhs_quadrature_points(C.byref(ma.c), int(order), None, None, C.byref(n))
    if st != 0:
        raise TpsRhsError(st, "tpsrhs_quadrature_points")
    xyz = np.zeros((host_mesh.dim, n.value))
    w = np.zeros(n.value)
    st = lib.tpsrhs_quadrature_points(C.byref(ma.c), int(order), xyz.ctypes.data, w.ctypes.data, C.byref(n))
    if st != 0:
        raise TpsRhsError(st, "tpsrhs_quadrature_points")
    return xyz, w


def node_coordinates(host_mesh, order: int, basis_type: int = 0) -> np.ndarray:
    """Physical coordinates of the DG nodes, ``(dim, NDofs)``: the role of
    ``mesh->GetNodes(*coordsDof)`` (``src/rhs_operator.cpp:139-142``) for a Gauss-Legendre (``basis_type`` 0) or
    Gauss-Lobatto (1) nodal basis on order-1 geometry.  Host-side input generation only."""
    dim = host_mesh.dim
    n1 = order + 1
    if basis_type == 0:
        x, _ = np.polynomial.legendre.leggauss(n1)
    else:  # end points and the roots of P'_{n1-1}
        inner = np.polynomial.legendre.Legendre.basis(n1 - 1).deriv().roots() if n1 > 2 else np.array([])
        x = np.concatenate([[-1.0], np.sort(inner.real), [1.0]])
    x = 0.5 * (x + 1.0)
    ex = host_mesh.elem_coords  # (ne, 2^dim, dim), MFEM order
    if dim == 3:
        corners = [(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1)]
        k, j, i = np.meshgrid(x, x, x, indexing="ij")
        xi = [i.ravel(), j.ravel(), k.ravel()]
    else:
        corners = [(0, 0), (1, 0), (1, 1), (0, 1)]
        j, i = np.meshgrid(x, x, indexing="ij")
        xi = [i.ravel(), j.ravel()]
    out = np.zeros((dim, host_mesh.num_elements, xi[0].size))
    for v, c in enumerate(corners):
        shp = np.ones_like(xi[0])
        for d in range(dim):
            shp = shp * (xi[d] if c[d] else 1.0 - xi[d])
        for d in range(dim):
            out[d] += ex[:, v, d][:, None] * shp[None, :]
    return out.reshape(dim, -1)
