// Point sampling of libtpsrhs.so (sampling.hpp, point_locate.hpp, locate_device.hpp): locating points, the lattice of a
// plane, samplers and tpsrhs_sample, node coordinates, the transfer between two operators, and the probe records -- an
// observer of the device time loop (abi_support.hpp: probe_cadence, probe_record).
#include "abi_support.hpp"
#include "locate_device.hpp"

#include <cmath>
#include <mutex>

namespace {
// the operator's sampling state, made at the first sampler or search grid
tpsrhs_sampling_state *sampling_of(tpsrhs_operator *h) {
  if (!h->sampling) h->sampling = owned_state(std::make_unique<tpsrhs_sampling_state>());
  return h->sampling.get();
}

void probe_off(tpsrhs_operator *h) {
  tpsrhs_sampling_state *ss = h->sampling.get();
  if (!ss || !ss->probe.sampler) return;
  (void)hipSetDevice(h->device);
  (void)hipStreamSynchronize(h->stream);  // a record may still be running
  ss->probe = tpsrhs_probe_log();
}

template <int DIM, int P>
void launch_sample(tpsrhs_operator *h, const tpsrhs_sampler *s, const SampleNodes &nodes, int nrows, const double *field,
                   double *out) {
  constexpr int BLOCK = 64;  // one wave: 64 probes are one block, a plane of 65 536 points is 1024 blocks over the 256 CUs
  const int64_t grid = (s->npts + BLOCK - 1) / BLOCK;
  if (grid == 0) return;
  if (grid >= (int64_t(1) << 31)) throw Unsupported("tpsrhs_sample: more than 2^37 points");
  hipLaunchKernelGGL((k_sample<DIM, P, BLOCK>), dim3(static_cast<unsigned>(grid)), dim3(BLOCK), 0, h->stream, s->npts, nrows,
                     h->ndofs, nodes, s->d_elem.get(), s->d_ref.get(), s->d_perm.get(), s->fill, field, out);
  HIP_CHECK(hipGetLastError());
}

// out[nrows][npts] = field[nrows][NDofs] at the points of s, on the operator's stream
void sample_field(tpsrhs_operator *h, const tpsrhs_sampler *s, int nrows, const double *field, double *out) {
  SampleNodes nodes = {};
  double wts[TPSRHS_MAXORDER + 1];
  segment_rule01(h->nc, h->order + 1, nodes.x, wts);  // the nodes of the operator's basis, as make_tables places them
  with_dim_order(h, "tpsrhs_sample", [&](auto dim, auto p) {
    launch_sample<decltype(dim)::value, decltype(p)::value>(h, s, nodes, nrows, field, out);
  });
}

// the position of s among the samplers of ss, or their end
auto sampler_find(tpsrhs_sampling_state *ss, const tpsrhs_sampler *s) {
  return std::find_if(ss->samplers.begin(), ss->samplers.end(), [s](const auto &u) { return u.get() == s; });
}

// s, a live sampler of h, leaves it
void sampler_remove(tpsrhs_operator *h, tpsrhs_sampler *s) {
  tpsrhs_sampling_state *ss = h->sampling.get();
  (void)hipSetDevice(h->device);
  (void)hipStreamSynchronize(h->stream);  // a sample may still be running
  if (ss->probe.sampler == s) probe_off(h);
  ss->samplers.erase(sampler_find(ss, s));
}

// The host copies of a device-located sampler (elem, ref, nfound), fetched once; synchronises the stream.
void sampler_fetch(tpsrhs_sampler *s) {
  if (s->host_valid) return;
  tpsrhs_operator *h = s->owner;
  HIP_CHECK(hipSetDevice(h->device));
  unsigned long long nf = 0;
  s->elem.resize(static_cast<size_t>(s->npts));
  s->ref.resize(static_cast<size_t>(s->npts) * h->dim);
  HIP_CHECK(hipMemcpyAsync(&nf, s->d_nfound.get(), sizeof(nf), hipMemcpyDeviceToHost, h->stream));
  if (s->npts) {
    HIP_CHECK(hipMemcpyAsync(s->elem.data(), s->d_elem.get(), s->elem.size() * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    HIP_CHECK(hipMemcpyAsync(s->ref.data(), s->d_ref.get(), s->ref.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  }
  HIP_CHECK(hipStreamSynchronize(h->stream));
  s->nfound = static_cast<int64_t>(nf);
  s->host_valid = true;
}
// ... and the count alone (tpsrhs_transfer's num_missing): 8 bytes instead of the arrays
int64_t sampler_nfound(tpsrhs_sampler *s) {
  if (s->host_valid) return s->nfound;
  tpsrhs_operator *h = s->owner;
  unsigned long long nf = 0;
  HIP_CHECK(hipMemcpyAsync(&nf, s->d_nfound.get(), sizeof(nf), hipMemcpyDeviceToHost, h->stream));
  HIP_CHECK(hipStreamSynchronize(h->stream));
  return static_cast<int64_t>(nf);
}

// The search grid of h's mesh for this tolerance on the device, built and uploaded at first use.
template <int DIM>
LocateGridView<DIM> device_grid(tpsrhs_operator *h, double tol) {
  tpsrhs_sampling_state *ss = sampling_of(h);
  tpsrhs_locate_grid_dev *g = nullptr;
  for (const auto &c : ss->grids)
    if (c->tol == tol) g = c.get();
  if (!g) {
    std::unique_ptr<tpsrhs_locate_grid_dev> up(new tpsrhs_locate_grid_dev());
    up->tol = tol;
    up->host = build_locate_grid<DIM>(h->ne, h->topo.verts.data(), tol);
    up->d_lo = DevBuf<double>(up->host.lo);
    up->d_hi = DevBuf<double>(up->host.hi);
    up->d_start = DevBuf<int64_t>(up->host.start);
    up->d_list = DevBuf<int32_t>(up->host.list);
    for (auto *v : {&up->host.lo, &up->host.hi}) std::vector<double>().swap(*v);
    std::vector<int64_t>().swap(up->host.start);
    std::vector<int32_t>().swap(up->host.list);
    g = up.get();
    ss->grids.push_back(std::move(up));
  }
  return locate_grid_view<DIM>(g->host, g->d_lo.get(), g->d_hi.get(), g->d_start.get(), g->d_list.get());
}

template <int DIM>
void launch_locate(tpsrhs_operator *h, tpsrhs_sampler *s, const double *xyz, double tol) {
  constexpr int BLOCK = 64;
  const int64_t grid = (s->npts + BLOCK - 1) / BLOCK;
  if (grid >= (int64_t(1) << 31)) throw Unsupported("tpsrhs_sampler_create_device: more than 2^37 points");
  const LocateGridView<DIM> g = device_grid<DIM>(h, tol);
  HIP_CHECK(hipMemsetAsync(s->d_nfound.get(), 0, sizeof(unsigned long long), h->stream));
  if (grid == 0) return;
  hipLaunchKernelGGL((k_locate<DIM, BLOCK>), dim3(static_cast<unsigned>(grid)), dim3(BLOCK), 0, h->stream, g, h->d_verts.get(), s->npts,
                     xyz, tol, s->d_elem.get(), s->d_ref.get(), s->d_perm.get(), s->d_nfound.get());
  HIP_CHECK(hipGetLastError());
}

// a sampler of h at the DEVICE points xyz[dim][npts], located on h's stream; registered with h
tpsrhs_sampler *sampler_create_device(tpsrhs_operator *h, int64_t npts, const double *xyz, double tol, double fill) {
  if (h->ne <= 0) throw Unsupported("tpsrhs_sampler_create_device: the operator has no elements");
  const double t = tol > 0.0 ? tol : LOCATE_DEFAULT_TOL;
  std::unique_ptr<tpsrhs_sampler> s(new tpsrhs_sampler());
  s->owner = h;
  s->npts = npts;
  s->fill = fill;
  s->on_device = true;
  s->host_valid = false;
  s->d_elem = DevBuf<int32_t>(npts);
  s->d_ref = DevBuf<double>(npts * h->dim);
  s->d_perm = DevBuf<int64_t>(npts);
  s->d_nfound = DevBuf<unsigned long long>(1);
  if (h->dim == 2)
    launch_locate<2>(h, s.get(), xyz, t);
  else
    launch_locate<3>(h, s.get(), xyz, t);
  h->sampling->samplers.push_back(std::move(s));  // exists: device_grid made it
  return h->sampling->samplers.back().get();
}

void node_coordinates_device(tpsrhs_operator *h, double *xyz_out, hipStream_t stream) {
  SampleNodes nodes = {};
  double wts[TPSRHS_MAXORDER + 1];
  segment_rule01(h->nc, h->order + 1, nodes.x, wts);  // as sample_field
  constexpr int BLOCK = 256;
  const int64_t grid = (h->ndofs + BLOCK - 1) / BLOCK;
  if (grid == 0) return;
  if (grid >= (int64_t(1) << 31)) throw Unsupported("tpsrhs_node_coordinates: more than 2^39 nodes");
  if (h->dim == 2)
    hipLaunchKernelGGL((k_node_coordinates<2, BLOCK>), dim3(static_cast<unsigned>(grid)), dim3(BLOCK), 0, stream, h->ndofs,
                       h->order + 1, nodes, h->d_verts.get(), xyz_out);
  else
    hipLaunchKernelGGL((k_node_coordinates<3, BLOCK>), dim3(static_cast<unsigned>(grid)), dim3(BLOCK), 0, stream, h->ndofs,
                       h->order + 1, nodes, h->d_verts.get(), xyz_out);
  HIP_CHECK(hipGetLastError());
}

// is s a live sampler?  (its owner is then s->owner)
bool sampler_alive(const tpsrhs_sampler *s, const tpsrhs_operator *h) {
  tpsrhs_sampling_state *ss = h ? h->sampling.get() : nullptr;
  return ss && sampler_find(ss, s) != ss->samplers.end();
}

// The sources of tpsrhs_transfer that hold a cached sampler: the destruction of ANY operator looks here for samplers at
// its nodes (the cache is keyed by the address of dst, which the next tpsrhs_create may hand out again).
std::mutex g_transfer_mu;
std::vector<tpsrhs_operator *> g_transfer_sources;
}  // namespace

// h is being destroyed: forget it as a source (its samplers go with its sampling state) and drop every sampler at its nodes
void transfer_forget(tpsrhs_operator *h) {
  std::lock_guard<std::mutex> lock(g_transfer_mu);
  auto &src = g_transfer_sources;
  src.erase(std::remove(src.begin(), src.end(), h), src.end());
  for (tpsrhs_operator *o : src) {
    auto &tr = o->sampling->transfers;  // exists: o holds a cached sampler
    for (size_t k = tr.size(); k-- > 0;)
      if (tr[k].dst == h) {
        sampler_remove(o, tr[k].sampler);
        tr.erase(tr.begin() + static_cast<std::ptrdiff_t>(k));
      }
  }
}

StepCadence *probe_cadence(tpsrhs_operator *h) { return h->sampling ? &h->sampling->probe.cadence : nullptr; }

// One probe record of the device vector x, stream-ordered, or one more dropped record when the buffer is full.
void probe_record(tpsrhs_operator *h, const double *x) {
  tpsrhs_probe_log &log = h->sampling->probe;
  const int64_t r = log.index.claim(log.cadence.count);
  if (r < 0) return;
  const int64_t per = static_cast<int64_t>(h->neq) * log.sampler->npts;
  sample_field(h, log.sampler, h->neq, x, log.d_values.get() + r * per);
  HIP_CHECK(hipMemcpyAsync(log.d_times.get() + r, h->loop.d_ctl.get() + 1, sizeof(double), hipMemcpyDeviceToDevice, h->stream));
}

extern "C" {

int tpsrhs_locate_points(const tpsrhs_mesh *mesh, int64_t npts, const double *xyz, double tol, int32_t *elem_out,
                         double *ref_out) {
  const int st = locate_points(mesh, npts, xyz, tol, elem_out, ref_out);
  if (st != TPSRHS_OK)
    return fail(st, "tpsrhs_locate_points: needs a mesh of dim 2 or 3 with elem_coords, npts >= 0, non-NULL arrays and a tolerance that is a number");
  return st;
}

int tpsrhs_plane_points(const double point[3], const double normal[3], const double bb0[3], const double bb1[3], int n,
                        double *xyz_out) {
  const int st = plane_points(point, normal, bb0, bb1, n, xyz_out);
  if (st != TPSRHS_OK) return fail(st, "tpsrhs_plane_points: needs non-NULL arguments and n >= 2");
  return st;
}

int tpsrhs_sampler_create(tpsrhs_handle h, int64_t npts, const double *xyz, double tol, double fill,
                          tpsrhs_sampler_handle *out) {
  if (out) *out = nullptr;
  if (!h || !out || npts < 0 || (npts > 0 && !xyz) || std::isnan(tol))
    return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_sampler_create: needs a handle, npts >= 0, the points and a tolerance that is a number");
  return guarded([&] {
    HIP_CHECK(hipSetDevice(h->device));
    const int dim = h->dim;
    std::unique_ptr<tpsrhs_sampler> sp(new tpsrhs_sampler());
    sp->owner = h;
    sp->npts = npts;
    sp->fill = fill;
    sp->elem.assign(static_cast<size_t>(npts), -1);
    sp->ref.assign(static_cast<size_t>(npts) * dim, 0.0);
    // the operator's own host copy of the element vertices (Topology::verts, already in lexicographic corner order)
    const double t = tol > 0.0 ? tol : LOCATE_DEFAULT_TOL;
    if (dim == 2)
      locate_points_lex<2>(h->ne, h->topo.verts.data(), npts, xyz, t, sp->elem.data(), sp->ref.data());
    else
      locate_points_lex<3>(h->ne, h->topo.verts.data(), npts, xyz, t, sp->elem.data(), sp->ref.data());
    // sorted by element, ties in the caller's order, the points that were not found last
    std::vector<int64_t> perm(static_cast<size_t>(npts));
    for (int64_t i = 0; i < npts; i++) perm[static_cast<size_t>(i)] = i;
    const std::vector<int32_t> &el = sp->elem;
    std::stable_sort(perm.begin(), perm.end(), [&](int64_t a, int64_t b) {
      const int64_t ea = el[static_cast<size_t>(a)] < 0 ? int64_t(1) << 40 : el[static_cast<size_t>(a)];
      const int64_t eb = el[static_cast<size_t>(b)] < 0 ? int64_t(1) << 40 : el[static_cast<size_t>(b)];
      return ea < eb;
    });
    std::vector<int32_t> selem(static_cast<size_t>(npts));
    std::vector<double> sref(static_cast<size_t>(npts) * dim);
    for (int64_t k = 0; k < npts; k++) {
      const int64_t i = perm[static_cast<size_t>(k)];
      selem[static_cast<size_t>(k)] = el[static_cast<size_t>(i)];
      if (el[static_cast<size_t>(i)] >= 0) sp->nfound++;
      for (int d = 0; d < dim; d++) sref[static_cast<size_t>(k + d * npts)] = sp->ref[static_cast<size_t>(i + d * npts)];
    }
    sp->d_elem = DevBuf<int32_t>(selem);
    sp->d_ref = DevBuf<double>(sref);
    sp->d_perm = DevBuf<int64_t>(perm);
    tpsrhs_sampling_state *ss = sampling_of(h);
    ss->samplers.push_back(std::move(sp));
    *out = ss->samplers.back().get();
  });
}

int tpsrhs_sampler_destroy(tpsrhs_sampler_handle s) {
  if (!s) return TPSRHS_OK;
  tpsrhs_operator *h = s->owner;
  if (!sampler_alive(s, h)) return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_sampler_destroy: not a sampler of a live operator");
  sampler_remove(h, s);
  return TPSRHS_OK;
}

int tpsrhs_sampler_info(tpsrhs_sampler_handle s, int64_t *npts, int64_t *nfound, int32_t *elem_out, double *ref_out) {
  if (!s) return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_sampler_info: NULL sampler");
  if (!s->host_valid) {  // located on the device: the host copies come on demand
    const int st = guarded([&] { sampler_fetch(s); });
    if (st != TPSRHS_OK) return st;
  }
  if (npts) *npts = s->npts;
  if (nfound) *nfound = s->nfound;
  if (elem_out && s->npts) std::memcpy(elem_out, s->elem.data(), s->elem.size() * sizeof(int32_t));
  if (ref_out && s->npts) std::memcpy(ref_out, s->ref.data(), s->ref.size() * sizeof(double));
  return TPSRHS_OK;
}

int tpsrhs_sample(tpsrhs_sampler_handle s, int nrows, const double *field, double *out) {
  if (!s || !field || !out || nrows < 1)
    return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_sample: needs a sampler, nrows >= 1 and non-NULL device arrays");
  tpsrhs_operator *h = s->owner;
  return guarded([&] {
    HIP_CHECK(hipSetDevice(h->device));
    sample_field(h, s, nrows, field, out);
  });
}

int tpsrhs_sampler_create_device(tpsrhs_handle h, int64_t npts, const double *xyz, double tol, double fill,
                                 tpsrhs_sampler_handle *out) {
  if (out) *out = nullptr;
  if (!h || !out || npts < 0 || (npts > 0 && !xyz) || std::isnan(tol))
    return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_sampler_create_device: needs a handle, npts >= 0, the device points and a tolerance that is a number");
  return guarded([&] {
    HIP_CHECK(hipSetDevice(h->device));
    *out = sampler_create_device(h, npts, xyz, tol, fill);
  });
}

int tpsrhs_node_coordinates(tpsrhs_handle h, double *xyz_out) {
  if (!h || !xyz_out) return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_node_coordinates: NULL argument");
  return guarded([&] {
    HIP_CHECK(hipSetDevice(h->device));
    node_coordinates_device(h, xyz_out, h->stream);
  });
}

int tpsrhs_transfer(tpsrhs_handle src, tpsrhs_handle dst, int nrows, const double *field_src, double *field_dst, double tol,
                    double fill, int64_t *num_missing) {
  if (!src || !dst || !field_src || !field_dst || nrows < 1 || std::isnan(tol))
    return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_transfer: needs two operators, nrows >= 1, non-NULL device arrays and a tolerance that is a number");
  if (src->dim != dst->dim)
    return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_transfer: the operators differ in dim");
  if (src->device != dst->device)
    return fail(TPSRHS_ERR_UNSUPPORTED, "tpsrhs_transfer: the operators are on different devices");
  return guarded([&] {
    HIP_CHECK(hipSetDevice(src->device));
    const double t = tol > 0.0 ? tol : LOCATE_DEFAULT_TOL;
    tpsrhs_sampler *s = nullptr;
    {
      std::lock_guard<std::mutex> lock(g_transfer_mu);
      if (src->sampling)
        for (const tpsrhs_transfer_entry &e : src->sampling->transfers)
          if (e.dst == dst && e.tol == t) s = e.sampler;
      if (s) {
        src->sampling->num_cache_hits++;
      } else {
        // the nodes of dst, on src's stream (they depend on nothing dst's stream writes), live until they are located
        const DevBuf<double> xyz(static_cast<size_t>(dst->ndofs) * dst->dim);
        node_coordinates_device(dst, xyz.get(), src->stream);
        s = sampler_create_device(src, dst->ndofs, xyz.get(), t, fill);
        HIP_CHECK(hipStreamSynchronize(src->stream));  // once per pair: xyz is freed below
        src->sampling->transfers.push_back({dst, t, s});
        src->sampling->num_located++;
        if (std::find(g_transfer_sources.begin(), g_transfer_sources.end(), src) == g_transfer_sources.end())
          g_transfer_sources.push_back(src);
      }
    }
    s->fill = fill;
    sample_field(src, s, nrows, field_src, field_dst);
    if (dst->stream != src->stream) {  // dst's stream reads field_dst after this
      hipEvent_t ev;
      HIP_CHECK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
      hipError_t e1 = hipEventRecord(ev, src->stream);
      hipError_t e2 = e1 == hipSuccess ? hipStreamWaitEvent(dst->stream, ev, 0) : e1;
      (void)hipEventDestroy(ev);  // released when the record has completed
      HIP_CHECK(e2);
    }
    if (num_missing) *num_missing = s->npts - sampler_nfound(s);
  });
}

int tpsrhs_transfer_stats(tpsrhs_handle src, int64_t *num_located, int64_t *num_cache_hits) {
  if (!src) return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_transfer_stats: NULL handle");
  const tpsrhs_sampling_state *ss = src->sampling.get();
  if (num_located) *num_located = ss ? ss->num_located : 0;
  if (num_cache_hits) *num_cache_hits = ss ? ss->num_cache_hits : 0;
  return TPSRHS_OK;
}

int tpsrhs_probe_configure(tpsrhs_handle h, tpsrhs_sampler_handle s, int64_t interval, int64_t capacity) {
  if (!h) return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_probe_configure: NULL handle");
  if (interval < 0 || capacity < 0)
    return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_probe_configure: needs interval >= 0 (0: off) and capacity >= 0");
  const bool on = s != nullptr && interval > 0;
  if (on && capacity < 1) return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_probe_configure: needs capacity >= 1");
  if (on && (s->owner != h || !sampler_alive(s, h)))
    return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_probe_configure: the sampler belongs to another operator");
  return guarded([&] {
    probe_off(h);
    if (!on) return;
    HIP_CHECK(hipSetDevice(h->device));
    tpsrhs_probe_log log;
    log.sampler = s;
    log.cadence.interval = interval;
    log.index.capacity = capacity;
    log.d_values = DevBuf<double>(capacity * h->neq * s->npts);
    log.d_times = DevBuf<double>(capacity);
    loop_ctl(h);  // a record copies the time from there
    // complete: a call that throws above leaves the probes off.  (h->sampling exists: s is one of its samplers)
    h->sampling->probe = std::move(log);
  });
}

int tpsrhs_probe_read(tpsrhs_handle h, int64_t *nrecords, int64_t *ndropped, int64_t *iters_out, double *times_out,
                      double *values_out, int reset) {
  if (!h) return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_probe_read: NULL handle");
  tpsrhs_sampling_state *ss = h->sampling.get();
  if (!ss || !ss->probe.sampler) return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_probe_read: probes are not configured (tpsrhs_probe_configure)");
  return guarded([&] {
    HIP_CHECK(hipSetDevice(h->device));
    tpsrhs_probe_log &log = ss->probe;
    fetch_rows(h, times_out, log.d_times, log.index.nrecords, 1);
    fetch_rows(h, values_out, log.d_values, log.index.nrecords, static_cast<int64_t>(h->neq) * log.sampler->npts);
    HIP_CHECK(hipStreamSynchronize(h->stream));
    read_index(log.index, nrecords, ndropped, iters_out, reset);
  });
}

}  // extern "C"
