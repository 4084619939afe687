// Surface integrals over sets of element faces and the patch history of libtpsrhs.so (surface.hpp): tpsrhs_surface_create /
// _destroy / _info / _integrate and the history -- an observer of the device time loop (abi_support.hpp: surface_cadence,
// surface_record).  tpsrhs_patch_faces, the host selection, is with tpsrhs_wall_faces in wall_distance.hip.
#include <algorithm>
#include <mutex>
#include <numeric>
#include <unordered_set>

#include "abi_support.hpp"
#include "surface.hpp"

namespace {
void history_off(tpsrhs_operator *h) {
  tpsrhs_surface_state *ss = h->surface.get();
  if (!ss || !ss->history.surface) return;
  (void)hipSetDevice(h->device);
  (void)hipStreamSynchronize(h->stream);  // a record may still be running
  ss->history = tpsrhs_surface_log();
}

// Every live surface of every operator.  A handle names its operator (s->owner), but a handle whose operator is gone points
// into freed memory: the entry points that take a bare handle look here first and read nothing of a handle that is not listed.
std::mutex g_live_mu;
std::unordered_set<const tpsrhs_surface_s *> g_live;

bool surface_alive(const tpsrhs_surface_s *s) {
  std::lock_guard<std::mutex> lock(g_live_mu);
  return g_live.count(s) != 0;
}

// (the deleter runs in the operator's destructor: the surfaces an operator still holds die with it)
tpsrhs_surface_state *surfaces_of(tpsrhs_operator *h) {
  if (!h->surface)
    h->surface = OwnedState<tpsrhs_surface_state>(new tpsrhs_surface_state(), [](tpsrhs_surface_state *q) {
      {
        std::lock_guard<std::mutex> lock(g_live_mu);
        for (const auto &s : q->surfaces) g_live.erase(s.get());
      }
      delete q;
    });
  return h->surface.get();
}

std::vector<std::unique_ptr<tpsrhs_surface_s>>::iterator surface_find(tpsrhs_surface_state *ss, const tpsrhs_surface_s *s) {
  return std::find_if(ss->surfaces.begin(), ss->surfaces.end(), [&](const std::unique_ptr<tpsrhs_surface_s> &q) { return q.get() == s; });
}

// The sorted face list on the device and its runs: at most SURF_MAXBLOCKS full runs of whole batches, none across a patch
// boundary (a patch's last run may be short).
tpsrhs_surface_s *surface_create(tpsrhs_operator *h, int num_patches, int64_t nf, const std::vector<int32_t> &elem,
                                 const std::vector<int32_t> &face, const std::vector<int64_t> &per_patch) {
  if (nf >= (int64_t(1) << 31)) throw Unsupported("tpsrhs_surface_create: 2^31 faces or more");
  std::unique_ptr<tpsrhs_surface_s> s(new tpsrhs_surface_s());
  s->owner = h;
  s->num_patches = num_patches;
  s->num_faces = nf;
  s->faces_per_patch = per_patch;
  with_dim_order(h, "tpsrhs_surface_create", [&](auto dim, auto p) { s->fb = SurfCfg<decltype(dim)::value, decltype(p)::value>::FB; });
  // the rule and the 1-D tables: they depend on the operator's order and basis only
  const int n1 = h->order + 1, nq = quad_points_1d(h->order);
  double nodes[TPSRHS_MAXORDER + 1], wts[TPSRHS_MAXORDER + 1];
  segment_rule01(h->nc, n1, nodes, wts);  // the nodes of the operator's basis, as make_tables places them
  gauss_legendre01(nq, s->tab.g, s->tab.w);
  for (int q = 0; q < nq; q++)
    for (int a = 0; a < n1; a++) s->tab.B[q * n1 + a] = lagrange(nodes, n1, a, s->tab.g[q]);
  for (int side = 0; side < 2; side++)
    for (int a = 0; a < n1; a++) s->tab.L[side * n1 + a] = lagrange(nodes, n1, a, static_cast<double>(side));
  const int64_t batches = (nf + s->fb - 1) / s->fb;
  const int64_t run = std::max<int64_t>(1, (batches + SURF_MAXBLOCKS - 1) / SURF_MAXBLOCKS) * s->fb;
  std::vector<SurfaceRun> runs;
  std::vector<int32_t> patch_block(static_cast<size_t>(num_patches) + 1, 0);
  int64_t begin = 0;
  for (int p = 0; p < num_patches; p++) {
    patch_block[static_cast<size_t>(p)] = static_cast<int32_t>(runs.size());
    const int64_t end = begin + per_patch[static_cast<size_t>(p)];
    for (int64_t b = begin; b < end; b += run)
      runs.push_back({static_cast<int32_t>(b), static_cast<int32_t>(std::min(end, b + run))});
    begin = end;
  }
  patch_block[static_cast<size_t>(num_patches)] = static_cast<int32_t>(runs.size());
  s->nblocks = static_cast<int>(runs.size());
  s->d_elem = DevBuf<int32_t>(elem);
  s->d_face = DevBuf<int32_t>(face);
  s->d_runs = DevBuf<SurfaceRun>(runs);
  s->d_patch_block = DevBuf<int32_t>(patch_block);
  s->d_partial = DevBuf<double>(static_cast<size_t>(SURF_ACC) * std::max(s->nblocks, 1) * s->fb);
  tpsrhs_surface_state *ss = surfaces_of(h);
  ss->surfaces.push_back(std::move(s));
  {
    std::lock_guard<std::mutex> lock(g_live_mu);
    g_live.insert(ss->surfaces.back().get());
  }
  return ss->surfaces.back().get();
}

void surface_remove(tpsrhs_operator *h, tpsrhs_surface_s *s) {
  tpsrhs_surface_state *ss = h->surface.get();
  (void)hipSetDevice(h->device);
  if (ss->history.surface == s)
    history_off(h);
  else
    (void)hipStreamSynchronize(h->stream);  // an integral may still be running
  {
    std::lock_guard<std::mutex> lock(g_live_mu);
    g_live.erase(s);
  }
  ss->surfaces.erase(surface_find(ss, s));
}

// out[num_patches][nrows]([dim]) of the surface, on the operator's stream
void integrate_surface(tpsrhs_operator *h, tpsrhs_surface_s *s, int form, int nrows, const double *field, int64_t row_stride,
                       int64_t comp_stride, int radial, double *out) {
  const SurfTab &tab = s->tab;
  const int od = form == TPSRHS_SURFACE_NORMAL ? h->dim : 1;
  const int rows_per_pass = SURF_ACC / od;
  const int64_t np = static_cast<int64_t>(s->nblocks) * s->fb;
  for (int r0 = 0; r0 < nrows; r0 += rows_per_pass) {  // the stream orders the launches: one scratch serves every pass
    const int nr = std::min(rows_per_pass, nrows - r0);
    if (s->nblocks > 0) {
      with_dim_order(h, "tpsrhs_surface_integrate", [&](auto dim, auto p) {
        hipLaunchKernelGGL((k_surface<decltype(dim)::value, decltype(p)::value>), dim3(s->nblocks), dim3(64), 0, h->stream, form, nr,
                           row_stride, comp_stride, radial, tab, s->d_runs.get(), s->d_elem.get(), s->d_face.get(),
                           h->d_verts.get(), field + r0 * row_stride, s->d_partial.get());
      });
      HIP_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(k_surface_final<256>, dim3(1), dim3(256), 0, h->stream, s->num_patches, nr * od, s->fb, np,
                       s->d_patch_block.get(), s->d_partial.get(), static_cast<int64_t>(nrows) * od,
                       out + static_cast<int64_t>(r0) * od);
    HIP_CHECK(hipGetLastError());
  }
}
}  // namespace

StepCadence *surface_cadence(tpsrhs_operator *h) { return h->surface ? &h->surface->history.cadence : nullptr; }

// One record of the patch history of the device vector x, stream-ordered, or one more dropped record when the buffer is full.
void surface_record(tpsrhs_operator *h, const double *x) {
  tpsrhs_surface_log &log = h->surface->history;
  const int64_t r = log.index.claim(log.cadence.count);
  if (r < 0) return;
  tpsrhs_surface_s *s = log.surface;
  const int axisym = h->dim == 2 && h->nvel == 3;
  integrate_surface(h, s, TPSRHS_SURFACE_SCALAR, h->neq, x, h->ndofs, 0, axisym, log.d_integrals.get() + r * s->num_patches * h->neq);
  integrate_surface(h, s, TPSRHS_SURFACE_FLUX, 1, x + h->ndofs, 0, h->ndofs, axisym, log.d_mass_flow.get() + r * s->num_patches);
  HIP_CHECK(hipMemcpyAsync(log.d_times.get() + r, h->loop.d_ctl.get() + 1, sizeof(double), hipMemcpyDeviceToDevice, h->stream));
}

extern "C" {

int tpsrhs_surface_create(tpsrhs_handle h, int num_patches, int64_t num_faces, const int32_t *elem, const int32_t *face,
                          const int32_t *patch, tpsrhs_surface_handle *out) {
  if (out) *out = nullptr;
  if (!h || !out || num_patches < 1 || num_faces < 0 || (num_faces > 0 && (!elem || !face || !patch)))
    return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_surface_create: needs a handle, num_patches >= 1, num_faces >= 0 with the three host arrays, and out");
  if (num_faces > static_cast<int64_t>(h->ne) * 2 * h->dim)
    return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_surface_create: more faces than the mesh has (a duplicate (element, face))");
  for (int64_t i = 0; i < num_faces; i++) {
    if (elem[i] < 0 || elem[i] >= h->ne)
      return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_surface_create: face " + std::to_string(i) + ": element outside 0 .. ne-1");
    if (face[i] < 0 || face[i] >= 2 * h->dim)
      return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_surface_create: face " + std::to_string(i) + ": local face outside 0 .. 2 dim - 1");
    if (patch[i] < 0 || patch[i] >= num_patches)
      return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_surface_create: face " + std::to_string(i) + ": patch outside 0 .. num_patches-1");
  }
  // sorted by (patch, element, face); a duplicate (element, face) shows in the order by (element, face)
  std::vector<int64_t> perm(static_cast<size_t>(num_faces));
  std::iota(perm.begin(), perm.end(), int64_t(0));
  auto slot = [&](int64_t i) { return static_cast<int64_t>(elem[i]) * 2 * h->dim + face[i]; };
  std::sort(perm.begin(), perm.end(), [&](int64_t a, int64_t b) { return slot(a) < slot(b); });
  for (int64_t i = 1; i < num_faces; i++)
    if (slot(perm[static_cast<size_t>(i)]) == slot(perm[static_cast<size_t>(i - 1)]))
      return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_surface_create: element " + std::to_string(elem[perm[static_cast<size_t>(i)]]) +
                                                   ", local face " + std::to_string(face[perm[static_cast<size_t>(i)]]) + " is listed twice");
  std::stable_sort(perm.begin(), perm.end(), [&](int64_t a, int64_t b) { return patch[a] < patch[b]; });
  std::vector<int32_t> se(static_cast<size_t>(num_faces)), sf(static_cast<size_t>(num_faces));
  std::vector<int64_t> per_patch(static_cast<size_t>(num_patches), 0);
  for (int64_t i = 0; i < num_faces; i++) {
    const int64_t k = perm[static_cast<size_t>(i)];
    se[static_cast<size_t>(i)] = elem[k];
    sf[static_cast<size_t>(i)] = face[k];
    per_patch[static_cast<size_t>(patch[k])]++;
  }
  return guarded([&] {
    HIP_CHECK(hipSetDevice(h->device));
    *out = surface_create(h, num_patches, num_faces, se, sf, per_patch);
  });
}

int tpsrhs_surface_destroy(tpsrhs_surface_handle s) {
  if (!s) return TPSRHS_OK;
  if (!surface_alive(s)) return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_surface_destroy: not a surface of a live operator");
  surface_remove(s->owner, s);
  return TPSRHS_OK;
}

int tpsrhs_surface_info(tpsrhs_surface_handle s, int *num_patches, int64_t *num_faces, int64_t *faces_per_patch) {
  if (!s || !surface_alive(s)) return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_surface_info: not a surface of a live operator");
  if (num_patches) *num_patches = s->num_patches;
  if (num_faces) *num_faces = s->num_faces;
  if (faces_per_patch) std::copy(s->faces_per_patch.begin(), s->faces_per_patch.end(), faces_per_patch);
  return TPSRHS_OK;
}

int tpsrhs_surface_integrate(tpsrhs_surface_handle s, int form, int nrows, const double *field, int64_t row_stride,
                             int64_t comp_stride, int radial_weight, double *out) {
  if (!s || !field || !out || nrows < 1)
    return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_surface_integrate: needs a surface, nrows >= 1, the device field and the device output");
  if (!surface_alive(s)) return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_surface_integrate: not a surface of a live operator");
  if (form != TPSRHS_SURFACE_SCALAR && form != TPSRHS_SURFACE_FLUX && form != TPSRHS_SURFACE_NORMAL)
    return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_surface_integrate: form " + std::to_string(form) + " is none of SCALAR, FLUX, NORMAL");
  tpsrhs_operator *h = s->owner;
  return guarded([&] {
    HIP_CHECK(hipSetDevice(h->device));
    integrate_surface(h, s, form, nrows, field, row_stride, comp_stride, radial_weight ? 1 : 0, out);
  });
}

int tpsrhs_surface_loads(tpsrhs_surface_handle s, const double *x, int part, int gradients_current, double *out) {
  if (!s || !x || !out) return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_surface_loads: needs a surface, the device state and the device output");
  if (!surface_alive(s)) return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_surface_loads: not a surface of a live operator");
  if (part != TPSRHS_FLUX_TOTAL && part != TPSRHS_FLUX_CONVECTIVE && part != TPSRHS_FLUX_VISCOUS)
    return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_surface_loads: part " + std::to_string(part) + " is none of TOTAL, CONVECTIVE, VISCOUS");
  tpsrhs_operator *h = s->owner;
  return guarded([&] {
    HIP_CHECK(hipSetDevice(h->device));
    if (!s->d_flux) s->d_flux = DevBuf<double>(static_cast<size_t>(h->dim) * h->neq * h->ndofs);
    get_flux(h, x, part, gradients_current, s->d_flux.get());  // [d][eq][NDofs]: rows eq, components d
    integrate_surface(h, s, TPSRHS_SURFACE_FLUX, h->neq, s->d_flux.get(), h->ndofs, static_cast<int64_t>(h->neq) * h->ndofs,
                      (h->dim == 2 && h->nvel == 3) ? 1 : 0, out);
  });
}

int tpsrhs_surface_monitor_configure(tpsrhs_handle h, tpsrhs_surface_handle s, int64_t interval, int64_t capacity) {
  if (!h) return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_surface_monitor_configure: NULL handle");
  if (interval < 0 || capacity < 0)
    return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_surface_monitor_configure: needs interval >= 0 (0: off) and capacity >= 0");
  const bool on = s != nullptr && interval > 0;
  if (on && capacity < 1) return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_surface_monitor_configure: needs capacity >= 1");
  if (on && (!surface_alive(s) || s->owner != h))
    return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_surface_monitor_configure: the surface belongs to another operator");
  return guarded([&] {
    history_off(h);
    if (!on) return;
    HIP_CHECK(hipSetDevice(h->device));
    tpsrhs_surface_log log;
    log.surface = s;
    log.cadence.interval = interval;
    log.index.capacity = capacity;
    log.d_times = DevBuf<double>(capacity);
    log.d_integrals = DevBuf<double>(capacity * s->num_patches * h->neq);
    log.d_mass_flow = DevBuf<double>(capacity * s->num_patches);
    loop_ctl(h);  // a record copies the time from there
    // complete: a call that throws above leaves the history off.  (h->surface exists: s is one of its surfaces)
    h->surface->history = std::move(log);
  });
}

int tpsrhs_surface_monitor_read(tpsrhs_handle h, int64_t *nrecords, int64_t *ndropped, int64_t *iters_out, double *times_out,
                                double *integrals_out, double *mass_flow_out, int reset) {
  if (!h) return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_surface_monitor_read: NULL handle");
  tpsrhs_surface_state *ss = h->surface.get();
  if (!ss || !ss->history.surface)
    return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_surface_monitor_read: the patch history is not configured (tpsrhs_surface_monitor_configure)");
  return guarded([&] {
    HIP_CHECK(hipSetDevice(h->device));
    tpsrhs_surface_log &log = ss->history;
    const int64_t n = log.index.nrecords, np = log.surface->num_patches;
    fetch_rows(h, times_out, log.d_times, n, 1);
    fetch_rows(h, integrals_out, log.d_integrals, n, np * h->neq);
    fetch_rows(h, mass_flow_out, log.d_mass_flow, n, np);
    HIP_CHECK(hipStreamSynchronize(h->stream));
    read_index(log.index, nrecords, ndropped, iters_out, reset);
  });
}

}  // extern "C"
