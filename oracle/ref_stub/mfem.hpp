// TEST INFRASTRUCTURE, computes nothing but containers -- a stand-in for <mfem.hpp>, written from scratch, only so
// that the POINT-PHYSICS translation units of the reference (equation of state, transport, chemistry, fluxes, Riemann
// solver: oracle/ref.mk) compile into oracle/_ref/libtpsref_point.so without MFEM.  Those units use MFEM for three
// containers (Vector, DenseMatrix, Array), a few macros and POINTERS to mesh / finite-element classes they never
// dereference on the paths oracle/ref_point.cpp calls.  Everything below is either such a container or an empty
// declaration; no finite-element machinery is imitated, so nothing of the reference's assembled operator can be built
// against it.  No part of the product.
#ifndef TPSREF_STUB_MFEM_HPP_
#define TPSREF_STUB_MFEM_HPP_

#include <mpi.h>

#include <algorithm>
#include <cassert>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <iostream>
#include <list>
#include <map>
#include <string>
#include <unordered_map>
#include <vector>

#define MFEM_HOST_DEVICE
#define MFEM_VERIFY(c, m) assert(c)
#define MFEM_ASSERT(c, m) assert(c)
#define MFEM_ABORT(m) abort()
#define MFEM_FORALL(i, N, ...) \
  for (int i = 0; i < N; i++) { \
    __VA_ARGS__ \
  }
#define MFEM_FORALL_2D(i, N, X, Y, Z, ...) \
  for (int i = 0; i < N; i++) { \
    __VA_ARGS__ \
  }
#define MFEM_FOREACH_THREAD(i, k, N) for (int i = 0; i < N; i++)
#define MFEM_SYNC_THREAD
#define MFEM_SHARED

namespace mfem {

inline void mfem_error(const char *m = "") {
  std::cerr << m << std::endl;
  std::abort();
}

template <class T>
class Array {
 public:
  Array() {}
  explicit Array(int n) : d_(n) {}
  int Size() const { return static_cast<int>(d_.size()); }
  void SetSize(int n) { d_.resize(n); }
  T &operator[](int i) { return d_[i]; }
  const T &operator[](int i) const { return d_[i]; }
  void Append(const T &t) { d_.push_back(t); }
  void operator=(const T &v) { std::fill(d_.begin(), d_.end(), v); }
  T *GetData() { return d_.data(); }
  const T *Read() const { return d_.data(); }
  T *Write() { return d_.data(); }
  T *ReadWrite() { return d_.data(); }
  const T *HostRead() const { return d_.data(); }
  T *HostWrite() { return d_.data(); }
  T *HostReadWrite() { return d_.data(); }

 private:
  std::vector<T> d_;
};

class Vector {
 public:
  Vector() {}
  explicit Vector(int n) : d_(n, 0.0) {}
  Vector(double *p, int n) : d_(p, p + n) {}  // a COPY: the stub has no aliasing vectors
  int Size() const { return static_cast<int>(d_.size()); }
  void SetSize(int n) { d_.resize(n, 0.0); }
  double &operator()(int i) { return d_[i]; }
  const double &operator()(int i) const { return d_[i]; }
  double &operator[](int i) { return d_[i]; }
  const double &operator[](int i) const { return d_[i]; }
  Vector &operator=(double v) {
    std::fill(d_.begin(), d_.end(), v);
    return *this;
  }
  Vector &operator*=(double v) {
    for (double &x : d_) x *= v;
    return *this;
  }
  Vector &operator/=(double v) {
    for (double &x : d_) x /= v;
    return *this;
  }
  Vector &operator+=(const Vector &o) {
    for (size_t i = 0; i < d_.size(); i++) d_[i] += o.d_[i];
    return *this;
  }
  Vector &operator-=(const Vector &o) {
    for (size_t i = 0; i < d_.size(); i++) d_[i] -= o.d_[i];
    return *this;
  }
  double operator*(const Vector &o) const {
    double s = 0;
    for (size_t i = 0; i < d_.size(); i++) s += d_[i] * o.d_[i];
    return s;
  }
  double Norml2() const { return std::sqrt((*this) * (*this)); }
  double Sum() const {
    double s = 0;
    for (double x : d_) s += x;
    return s;
  }
  double Max() const { return *std::max_element(d_.begin(), d_.end()); }
  double Min() const { return *std::min_element(d_.begin(), d_.end()); }
  void Add(double a, const Vector &o) {
    for (size_t i = 0; i < d_.size(); i++) d_[i] += a * o.d_[i];
  }
  void Set(double a, const Vector &o) {
    d_ = o.d_;
    for (double &x : d_) x *= a;
  }
  void Print(std::ostream & = std::cout, int = 8) const {}
  void UseDevice(bool) {}
  double *GetData() const { return const_cast<double *>(d_.data()); }
  const double *Read() const { return d_.data(); }
  double *Write() { return d_.data(); }
  double *ReadWrite() { return d_.data(); }
  const double *HostRead() const { return d_.data(); }
  double *HostWrite() { return d_.data(); }
  double *HostReadWrite() { return d_.data(); }

 private:
  std::vector<double> d_;
};

class DenseMatrix {  // column-major, as MFEM's
 public:
  DenseMatrix() : h_(0), w_(0) {}
  DenseMatrix(int h, int w) { SetSize(h, w); }
  explicit DenseMatrix(int h) { SetSize(h, h); }
  void SetSize(int h, int w) {
    h_ = h;
    w_ = w;
    d_.assign(static_cast<size_t>(h) * w, 0.0);
  }
  void SetSize(int h) { SetSize(h, h); }
  int Height() const { return h_; }
  int Width() const { return w_; }
  int NumRows() const { return h_; }
  int NumCols() const { return w_; }
  double &operator()(int i, int j) { return d_[i + static_cast<size_t>(j) * h_]; }
  const double &operator()(int i, int j) const { return d_[i + static_cast<size_t>(j) * h_]; }
  DenseMatrix &operator=(double v) {
    std::fill(d_.begin(), d_.end(), v);
    return *this;
  }
  DenseMatrix &operator*=(double v) {
    for (double &x : d_) x *= v;
    return *this;
  }
  void Mult(const Vector &x, Vector &y) const {
    for (int i = 0; i < h_; i++) {
      double s = 0;
      for (int j = 0; j < w_; j++) s += (*this)(i, j) * x(j);
      y(i) = s;
    }
  }
  void GetRow(int r, Vector &v) const {
    v.SetSize(w_);
    for (int j = 0; j < w_; j++) v(j) = (*this)(r, j);
  }
  void GetColumn(int c, Vector &v) const {
    v.SetSize(h_);
    for (int i = 0; i < h_; i++) v(i) = (*this)(i, c);
  }
  void SetRow(int r, const Vector &v) {
    for (int j = 0; j < w_; j++) (*this)(r, j) = v(j);
  }
  void SetCol(int c, const Vector &v) {
    for (int i = 0; i < h_; i++) (*this)(i, c) = v(i);
  }
  double Trace() const {
    double s = 0;
    for (int i = 0; i < h_; i++) s += (*this)(i, i);
    return s;
  }
  void Print(std::ostream & = std::cout, int = 4) const {}
  double *GetData() const { return const_cast<double *>(d_.data()); }
  const double *Read() const { return d_.data(); }
  double *Write() { return d_.data(); }
  const double *HostRead() const { return d_.data(); }
  double *HostWrite() { return d_.data(); }

 private:
  int h_, w_;
  std::vector<double> d_;
};

// ---- names the reference's headers mention; only pointers and references to them are compiled -------------------
class DenseTensor;
class Mesh;
class ParMesh;
class FiniteElementCollection;
class IntegrationRule;
class IntegrationRules;
class DG_FECollection;
class H1_FECollection;
class ODESolver;
class ParaViewDataCollection;
class VisItDataCollection;
class DataCollection;
class NonlinearForm;
class ParNonlinearForm;

struct Ordering {
  enum Type { byNODES, byVDIM };
};
struct Mpi {
  static bool Root() { return true; }
  static int WorldRank() { return 0; }
  static int WorldSize() { return 1; }
};
class FiniteElementSpace {
 public:
  int GetNDofs() const { return 0; }
  int GetVDim() const { return 1; }
  int GetVSize() const { return 0; }
  Ordering::Type GetOrdering() const { return Ordering::byNODES; }
};
class ParFiniteElementSpace : public FiniteElementSpace {};
class GridFunction : public Vector {
 public:
  FiniteElementSpace *FESpace() const { return nullptr; }
};
class ParGridFunction : public GridFunction {
 public:
  ParFiniteElementSpace *ParFESpace() const { return nullptr; }
};
class IntegrationPoint {
 public:
  double x, y, z, weight;
};
class ElementTransformation {
 public:
  void Transform(const IntegrationPoint &, Vector &) {}
};
class Coefficient {
 public:
  virtual ~Coefficient() {}
  virtual double Eval(ElementTransformation &T, const IntegrationPoint &ip) = 0;
  void SetTime(double) {}
  double GetTime() { return 0; }
};
class VectorCoefficient {
 public:
  explicit VectorCoefficient(int vd = 0) : vdim(vd) {}
  virtual ~VectorCoefficient() {}
  virtual void Eval(Vector &V, ElementTransformation &T, const IntegrationPoint &ip) = 0;
  int GetVDim() { return vdim; }
  void SetTime(double) {}
  double GetTime() { return 0; }

 protected:
  int vdim;
};
class MatrixCoefficient {
 public:
  explicit MatrixCoefficient(int d = 0) : height(d), width(d) {}
  MatrixCoefficient(int h, int w) : height(h), width(w) {}
  virtual ~MatrixCoefficient() {}
  virtual void Eval(DenseMatrix &K, ElementTransformation &T, const IntegrationPoint &ip) = 0;
  int GetHeight() const { return height; }
  int GetWidth() const { return width; }
  void SetTime(double) {}
  double GetTime() { return 0; }

 protected:
  int height, width;
};
class Operator {
 public:
  explicit Operator(int s = 0) : height(s), width(s) {}
  virtual ~Operator() {}
  virtual void Mult(const Vector &x, Vector &y) const = 0;
  int Height() const { return height; }
  int Width() const { return width; }

 protected:
  int height, width;
};
class TimeDependentOperator : public Operator {
 public:
  explicit TimeDependentOperator(int n = 0, double t0 = 0) : Operator(n), t(t0) {}

 protected:
  double t;
};
class ConstrainedOperator : public Operator {
 public:
  void Mult(const Vector &, Vector &) const override {}
};
class Solver : public Operator {
 public:
  virtual void SetOperator(const Operator &) = 0;
};

}  // namespace mfem

using namespace mfem;  // the reference's sources rely on <mfem.hpp> having been followed by this in their own headers
#endif
