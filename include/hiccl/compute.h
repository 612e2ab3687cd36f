// include/hiccl/compute.h -- HiCCL::Compute<T>, the reduction compute stage.
//
// Same object contract as the reference (source/compute.h:26-204): add()
// registers one compute on its owning rank (SPMD filter, compute.h:66),
// start() launches every registered compute, wait() blocks until they are
// done, report()/measure() print the reference's tables.  The MI355X port
// keeps all registered computes in ONE hiccl_reduce_plan and start() is a
// single batched kernel launch on the process's compute stream (the
// reference launches one reduce_kernel per compute on a stream of its own,
// compute.h:87-106, and synchronises each, compute.h:107-117).
//
// Host port (HICCL_PORT_HOST, no GPU: config 1) runs the same in-order sum
// with OpenMP on host memory, like the reference's no-PORT build
// (compute.h:14-23).  It is selected at compile time; a HIP build contains no
// CPU reduction.
#ifndef HICCL_COMPUTE_H
#define HICCL_COMPUTE_H

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <type_traits>
#include <vector>

#include "elem_types.h"
#include "ops.h"
#include "transport.h"

#ifndef HICCL_PORT_HOST
#include "../hiccl_reduce.h"
#endif

namespace HiCCL {

// bf16 and f16, the 2-byte storage types, and f8e4m3 and f8e5m2, the 1-byte
// ones (OCP FP8): elem_types.h.  maxof<U>, minof<U>,
// prodof<U>, bandof<U>, borof<U>, bxorof<U>, the types whose `+=` is another
// operator: ops.h.

// T -> hiccl_dtype_t (an operator wrapper of U: U's; the operator is op_of<T>(), ops.h)
template <typename T>
constexpr int dtype_of() {
  if constexpr (op_of<T>() != 0) return dtype_of<typename op_traits<T>::value_type>();
  else if constexpr (std::is_same<T, float>::value) return 0;
  else if constexpr (std::is_same<T, double>::value) return 1;
  else if constexpr (std::is_integral<T>::value && sizeof(T) == 8) return 3;
  else if constexpr (std::is_integral<T>::value && sizeof(T) == 4) return 4;
  else if constexpr (std::is_same<T, bf16>::value) return 2;
  else if constexpr (std::is_same<T, f16>::value) return 6;
  else if constexpr (std::is_same<T, f8e4m3>::value) return 16;  // HICCL_FLOAT8_E4M3
  else if constexpr (std::is_same<T, f8e5m2>::value) return 17;  // HICCL_FLOAT8_E5M2
#ifdef __FLT16_MANT_DIG__  // the compiler has _Float16: its `+=` is the half add itself
  else if constexpr (std::is_same<T, _Float16>::value) return 6;
#endif
  else return -1;
}

// the dtypes a scaled sum takes: the floating ones
constexpr bool scalable_dtype(int d) { return d == 0 || d == 1 || d == 2 || d == 6 || d == 16 || d == 17; }

#ifndef HICCL_PORT_HOST
// One compute stream per process (see transport_stream()).
inline hipStream_t compute_stream() {
  static hipStream_t s = [] {
    hipStream_t t;
    CommBench::hip_check(hipStreamCreateWithFlags(&t, hipStreamNonBlocking), "hipStreamCreate(compute)");
    return t;
  }();
  return s;
}
#endif

template <typename T>
class Compute {
 public:
  int numcomp = 0;
  std::vector<std::vector<T *>> inputbuf;
  std::vector<T *> outputbuf;
  std::vector<size_t> count;

  Compute() {}
  ~Compute() {
#ifndef HICCL_PORT_HOST
    if (plan) hiccl_reduce_plan_destroy(plan);
#endif
  }
  Compute(const Compute &) = delete;
  Compute &operator=(const Compute &) = delete;

  // compute.h:47-85.  Every rank calls add; the owning rank records.
  // `peer_inputs`: some input is a peer GPU's buffer read in place (fused
  // gather): the step's kernel then loads with system scope
  // (hiccl_reduce_plan_set_peer).
  // `unscaled`: this compute writes the plain sum whatever the scale
  // (hiccl_reduce_plan_add_unscaled) -- an intermediate compute of an
  // averaging Comm<T> step, next to the final ones in the same launch.
  void add(std::vector<T *> &in, T *out, size_t n, int compid, bool peer_inputs = false, bool unscaled = false) {
    if (CommBench::myid != compid) return;
    inputbuf.push_back(in);
    outputbuf.push_back(out);
    count.push_back(n);
    plain.push_back(unscaled ? 1 : 0);
    numcomp++;
#ifndef HICCL_PORT_HOST
    static_assert(dtype_of<T>() >= 0, "HiCCL::Compute: unsupported element type");
    if (!plan) {
      check(hiccl_reduce_plan_create(&plan, dtype_of<T>(), CommBench::mydevice), "plan_create");
      // T = maxof<U> ... bxorof<U>: the plan runs U's kernels of that operator (a step
      // program takes the operator from the plan it records)
      if (op_of<T>() != HICCL_OP_SUM) check(hiccl_reduce_plan_set_op(plan, op_of<T>()), "plan_set_op");
      // HICCL_ENGINE=tile|phase|auto pins the kernel engine (same bits either
      // way, so ranks need not agree); default auto.
      if (const char *e = std::getenv("HICCL_ENGINE")) {
        const std::string v(e);
        const int eng = v == "tile" ? HICCL_ENGINE_TILE : v == "phase" ? HICCL_ENGINE_PHASE : HICCL_ENGINE_AUTO;
        check(hiccl_reduce_plan_set_engine(plan, eng), "plan_set_engine");
      }
      if (scaled) check(hiccl_reduce_plan_set_scale(plan, &scale), "plan_set_scale");  // set before the first add
    }
    if (peer_inputs && !(hiccl_reduce_plan_peer(plan) & HICCL_PEER_LOADS))
      check(hiccl_reduce_plan_set_peer(plan, hiccl_reduce_plan_peer(plan) | HICCL_PEER_LOADS), "plan_set_peer");
    if (unscaled)
      check(hiccl_reduce_plan_add_unscaled(plan, out, (const void *const *)in.data(), (int)in.size(), n), "plan_add_unscaled");
    else
      check(hiccl_reduce_plan_add(plan, out, (const void *const *)in.data(), (int)in.size(), n), "plan_add");
#else
    (void)peer_inputs;
#endif
  }

  // Scaled sums: every compute writes finish(sum, alpha) from the next
  // start() on (an average: alpha = 1 / inputs) -- in the sum's own pass, the
  // multiply once per element at store time (hiccl_reduce_plan_set_scale; the
  // host port applies the same scale_finish after host_sum, same bits).
  // Floating T only; alpha must be finite.  A compute added `unscaled` keeps
  // writing the plain sum: Comm<T>::set_scale builds its steps from both kinds.
  void set_scale(double alpha) {
    static_assert(op_of<T>() == 0, "HiCCL::Compute::set_scale: only sums are scaled (T is an operator wrapper)");
    static_assert(scalable_dtype(dtype_of<T>()),
                  "HiCCL::Compute::set_scale: floating element types only (float, double, bf16, f16, _Float16, "
                  "f8e4m3, f8e5m2)");
    if (!std::isfinite(alpha) || (!std::is_same<T, double>::value && !std::isfinite((float)alpha)))
      CommBench::die("Compute::set_scale", "alpha must be finite");
    scaled = true;
    scale = alpha;
#ifndef HICCL_PORT_HOST
    if (plan) check(hiccl_reduce_plan_set_scale(plan, &scale), "plan_set_scale");
#endif
  }
  void clear_scale() {
    scaled = false;
#ifndef HICCL_PORT_HOST
    if (plan) check(hiccl_reduce_plan_set_scale(plan, nullptr), "plan_set_scale");
#endif
  }

  // compute.h:87-106: nonblocking launch of all registered computes.
  void start() {
    if (!numcomp) return;
#ifndef HICCL_PORT_HOST
    check(hiccl_reduce_plan_launch(plan, compute_stream()), "plan_launch");
#else
    for (int c = 0; c < numcomp; c++) host_sum(outputbuf[c], count[c], inputbuf[c], scaled && !plain[c], scale);
#endif
  }

#ifndef HICCL_PORT_HOST
  // Stream-ordered execution: enqueue the step's batched kernel on `s`.
  void launch(hipStream_t s) {
    if (!numcomp) return;
    CommBench::flush_signals();  // queued signal/wait steps precede this kernel on the stream
    if (CommBench::step_recorder()) return CommBench::record_plan(plan, 2, this);  // a step program's element
    check(hiccl_reduce_plan_enqueue(plan, s), "plan_enqueue");  // the caller syncs the stream
  }
#endif

  // Algorithmic bytes of one start(): sum of count * (n + 1) * sizeof(T)
  // (the compute.h:197-203 accounting).
  size_t bytes() const {
    size_t b = 0;
    for (int c = 0; c < numcomp; c++) b += count[c] * (inputbuf[c].size() + 1) * sizeof(T);
    return b;
  }

  // compute.h:107-117
  void wait() {
#ifndef HICCL_PORT_HOST
    if (numcomp) check(hiccl_reduce_plan_sync(plan), "plan_sync");
#endif
  }

  // compute.h:119-135
  void report() {
    std::vector<int> nc(CommBench::numproc), ni(CommBench::numproc);
    int numinput = 0;
    for (auto &v : inputbuf) numinput += (int)v.size();
    MPI_Allgather(&numcomp, 1, MPI_INT, nc.data(), 1, MPI_INT, CommBench::comm_mpi);
    MPI_Allgather(&numinput, 1, MPI_INT, ni.data(), 1, MPI_INT, CommBench::comm_mpi);
    if (CommBench::myid == CommBench::printid) {
      std::printf("numcomp: ");
      for (int p = 0; p < CommBench::numproc; p++) std::printf("%d(%d) ", nc[p], ni[p]);
      std::printf("\n\n");
    }
  }

  // compute.h:137-196: time start()+wait() with barriers, MAX over ranks,
  // price `count` elements (the caller's choice, as the reference does).
  void measure(int warmup, int numiter, size_t cnt) {
    report();
    unsigned long busiest = 0;  // algorithmic bytes (n reads + 1 write) of the busiest rank
    for (int c = 0; c < numcomp; c++) busiest += (unsigned long)(count[c] * (inputbuf[c].size() + 1) * sizeof(T));
    MPI_Allreduce(MPI_IN_PLACE, &busiest, 1, MPI_UNSIGNED_LONG, MPI_MAX, CommBench::comm_mpi);
    roofline_bytes = (double)busiest;
    std::vector<double> times;
    if (CommBench::myid == CommBench::printid) {
      std::printf("Measure Reduction Kernel\n%d warmup iterations (in order)\n", warmup);
    }
    for (int it = -warmup; it < numiter; it++) {
#ifndef HICCL_PORT_HOST
      CommBench::hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");
#endif
      MPI_Barrier(CommBench::comm_mpi);
      double t0 = MPI_Wtime();
      start();
      double st = MPI_Wtime() - t0;
      wait();
      double t = MPI_Wtime() - t0;
      MPI_Allreduce(MPI_IN_PLACE, &st, 1, MPI_DOUBLE, MPI_MAX, CommBench::comm_mpi);
      MPI_Allreduce(MPI_IN_PLACE, &t, 1, MPI_DOUBLE, MPI_MAX, CommBench::comm_mpi);
      if (it < 0) {
        if (CommBench::myid == CommBench::printid) std::printf("startup %.2e warmup: %e\n", st, t);
      } else {
        times.push_back(t);
      }
    }
    print_times(times, (double)cnt * sizeof(T));
    roofline_bytes = 0;
  }

  // compute.h:197-203: price reads + writes, sum over ranks.  Also prints
  // the per-GPU HBM roofline fraction: the busiest rank's algorithmic bytes
  // over the median time against the 8 TB/s MI355X peak.
  void measure(int warmup, int numiter) {
    size_t tot = 0;
    for (int c = 0; c < numcomp; c++) tot += count[c] * (inputbuf[c].size() + 1);
    MPI_Allreduce(MPI_IN_PLACE, &tot, 1, MPI_UNSIGNED_LONG, MPI_SUM, CommBench::comm_mpi);
    measure(warmup, numiter, tot);
  }

  static constexpr double hbm_peak = 8.0e12;  // MI355X HBM3E, bytes/s

  static void print_times(std::vector<double> &times, double data) {
    if (times.empty() || CommBench::myid != CommBench::printid) return;
    std::sort(times.begin(), times.end());
    const int n = (int)times.size();
    std::printf("%d measurement iterations (sorted):\n", n);
    for (int i = 0; i < n; i++)
      std::printf("time: %.4e%s\n", times[i], i == 0 ? " -> min" : i == n / 2 ? " -> median" : i == n - 1 ? " -> max" : "");
    double avg = 0;
    for (double t : times) avg += t;
    avg /= n;
    std::printf("\ndata: ");
    CommBench::print_data((size_t)data);
    std::printf("\n");
    const double v[4] = {times[0], times[n / 2], times[n - 1], avg};
    const char *name[4] = {"min", "med", "max", "avg"};
    for (int i = 0; i < 4; i++)
      std::printf("%sTime: %.4e us, %.4e ms/GB, %.4e GB/s\n", name[i], v[i] * 1e6, v[i] / data * 1e12, data / v[i] / 1e9);
#ifndef HICCL_PORT_HOST
    if (roofline_bytes > 0)
      std::printf("HBM roofline (busiest rank, median): %.1f GB/s = %.1f %% of %.0f GB/s\n",
                  roofline_bytes / v[1] / 1e9, 100.0 * roofline_bytes / v[1] / hbm_peak, hbm_peak / 1e9);
#endif
    std::printf("\n");
  }

  static inline double roofline_bytes = 0;  // set by measure(warmup, numiter)

 private:
  bool scaled = false;  // set_scale / clear_scale
  double scale = 1.0;
  std::vector<char> plain;  // per compute: added unscaled
#ifndef HICCL_PORT_HOST
  hiccl_reduce_plan_t *plan = nullptr;
  static void check(int e, const char *what) {
    if (e) CommBench::die(what, hiccl_last_error());
  }
#else
  static void host_sum(T *out, size_t n, const std::vector<T *> &in, bool scaled, double alpha) {
    const int k = (int)in.size();
#pragma omp parallel for schedule(static)
    for (size_t i = 0; i < n; i++) {
      T acc = 0;
      for (int j = 0; j < k; j++) acc += in[j][i];
      if constexpr (op_of<T>() == 0 && scalable_dtype(dtype_of<T>())) {
        if (scaled) acc = scale_finish<T>(acc, alpha);
      }
      out[i] = acc;
    }
  }
#endif
};

// HiCCL::WidenCompute<T>: Compute's object contract for a WIDENED sum -- T
// inputs (bf16, f16 / _Float16, f8e4m3, f8e5m2), float outputs: every compute
// writes the in-order f32 sum of its widened inputs, the f32 accumulator as it
// is (hiccl_reduce_plan_set_out_dtype; low-precision gradient buckets into f32
// master gradients in one pass).  set_scale multiplies once in f32 at store
// time.  An output may not overlap an input.  The host port does the same
// arithmetic in plain C++ (widen_sum, elem_types.h): the same bits.
// set_accumulate makes every start() ADD to the outputs instead of overwriting
// them (hiccl_reduce_plan_set_accumulate): out = fl32(out + r), r the finished
// (and scaled) sum -- an f32 master gradient accumulated over micro-batches.
// add(in, out, n, compid, weights) makes the object WEIGHTED
// (hiccl_reduce_plan_set_weighted): input k of the compute counts as
// fl32(weights[k] * widen(x)), the product and the add rounded separately.  The
// weights are in.size() floats in DEVICE memory that every start() reads anew
// (on the host port: host memory, read by start() likewise).  The first add
// decides: an object takes weighted adds only, or none.
// A Comm<T> schedule has no use for it (a schedule moves T between ranks, and
// a widened sum changes type inside the tree: INTEGRATION.md).
template <typename T>
class WidenCompute {
  static_assert(widenable<T>(), "HiCCL::WidenCompute: bf16, f16 (_Float16), f8e4m3 or f8e5m2 inputs only");

 public:
  int numcomp = 0;
  std::vector<std::vector<T *>> inputbuf;
  std::vector<float *> outputbuf;
  std::vector<size_t> count;

  WidenCompute() {}
  ~WidenCompute() {
#ifndef HICCL_PORT_HOST
    if (plan) hiccl_reduce_plan_destroy(plan);
#endif
  }
  WidenCompute(const WidenCompute &) = delete;
  WidenCompute &operator=(const WidenCompute &) = delete;

  // As Compute<T>::add, with a float output.
  void add(std::vector<T *> &in, float *out, size_t n, int compid, bool peer_inputs = false) {
    add_impl(in, out, n, compid, nullptr, false, peer_inputs);
  }

  // The weighted form: `weights` are in.size() floats (device memory; host
  // memory on the host port), kept by pointer and read by every start().
  void add(std::vector<T *> &in, float *out, size_t n, int compid, const float *weights, bool peer_inputs = false) {
    add_impl(in, out, n, compid, weights, true, peer_inputs);
  }

 private:
  void add_impl(std::vector<T *> &in, float *out, size_t n, int compid, const float *weights, bool with_weights,
                bool peer_inputs) {
    if (CommBench::myid != compid) return;
    if (numcomp && with_weights != weighted)
      CommBench::die("WidenCompute::add", weighted ? "a weighted object takes weighted adds only (the first add decided)"
                                                   : "the object is not weighted (the first add decided)");
    weighted = with_weights;
    weightbuf.push_back(weights);
    inputbuf.push_back(in);
    outputbuf.push_back(out);
    count.push_back(n);
    numcomp++;
#ifndef HICCL_PORT_HOST
    if (!plan) {
      check(hiccl_reduce_plan_create(&plan, dtype_of<T>(), CommBench::mydevice), "plan_create");
      if (const char *e = std::getenv("HICCL_ENGINE")) {
        const std::string v(e);
        const int eng = v == "tile" ? HICCL_ENGINE_TILE : v == "phase" ? HICCL_ENGINE_PHASE : HICCL_ENGINE_AUTO;
        check(hiccl_reduce_plan_set_engine(plan, eng), "plan_set_engine");
      }
      check(hiccl_reduce_plan_set_out_dtype(plan, HICCL_FLOAT32), "plan_set_out_dtype");  // before the first add
      if (weighted) check(hiccl_reduce_plan_set_weighted(plan, 1), "plan_set_weighted");  // likewise
      if (scaled) check(hiccl_reduce_plan_set_scale(plan, &scale), "plan_set_scale");
      if (accumulating) check(hiccl_reduce_plan_set_accumulate(plan, 1), "plan_set_accumulate");
    }
    if (peer_inputs && !(hiccl_reduce_plan_peer(plan) & HICCL_PEER_LOADS))
      check(hiccl_reduce_plan_set_peer(plan, hiccl_reduce_plan_peer(plan) | HICCL_PEER_LOADS), "plan_set_peer");
    if (weighted)
      check(hiccl_reduce_plan_add_weighted(plan, out, (const void *const *)in.data(), weights, (int)in.size(), n),
            "plan_add_weighted");
    else
      check(hiccl_reduce_plan_add(plan, out, (const void *const *)in.data(), (int)in.size(), n), "plan_add");
#else
    (void)peer_inputs;
#endif
  }

 public:

  // out = fl32(sum * (float)alpha) from the next start() on; alpha finite, as a float too.
  void set_scale(double alpha) {
    if (!std::isfinite(alpha) || !std::isfinite((float)alpha)) CommBench::die("WidenCompute::set_scale", "alpha must be finite");
    scaled = true;
    scale = alpha;
#ifndef HICCL_PORT_HOST
    if (plan) check(hiccl_reduce_plan_set_scale(plan, &scale), "plan_set_scale");
#endif
  }
  void clear_scale() {
    scaled = false;
#ifndef HICCL_PORT_HOST
    if (plan) check(hiccl_reduce_plan_set_scale(plan, nullptr), "plan_set_scale");
#endif
  }

  // out = fl32(out + r) from the next start() on, r the sum (times the scale):
  // every start() accumulates once more.  At any time; false: overwrite again.
  void set_accumulate(bool on = true) {
    accumulating = on;
#ifndef HICCL_PORT_HOST
    if (plan) check(hiccl_reduce_plan_set_accumulate(plan, on ? 1 : 0), "plan_set_accumulate");
#endif
  }

  void start() {
    if (!numcomp) return;
#ifndef HICCL_PORT_HOST
    check(hiccl_reduce_plan_launch(plan, compute_stream()), "plan_launch");
#else
    for (int c = 0; c < numcomp; c++) {
      float *out = outputbuf[c];
      T *const *in = inputbuf[c].data();
      const int k = (int)inputbuf[c].size();
      const size_t n = count[c];
      const float *w = weightbuf[c];
      if (accumulating) {
#pragma omp parallel for schedule(static)
        for (size_t i = 0; i < n; i++) {
          // r in a statement of its own (and volatile, as widen_sum's partial
          // sums): a contracting compiler cannot fuse the multiply with the add
          volatile float r = weighted ? weighted_widen_sum<T>(in, w, k, i, scaled, scale) : widen_sum<T>(in, k, i, scaled, scale);
          out[i] = out[i] + r;
        }
      } else {
#pragma omp parallel for schedule(static)
        for (size_t i = 0; i < n; i++)
          out[i] = weighted ? weighted_widen_sum<T>(in, w, k, i, scaled, scale) : widen_sum<T>(in, k, i, scaled, scale);
      }
    }
#endif
  }

  void wait() {
#ifndef HICCL_PORT_HOST
    if (numcomp) check(hiccl_reduce_plan_sync(plan), "plan_sync");
#endif
  }

  // Algorithmic bytes of one start(): sum of count * (n * sizeof(T) + 4); an
  // accumulating compute also reads its output: + 8.
  size_t bytes() const {
    const size_t obytes = accumulating ? 2 * sizeof(float) : sizeof(float);
    size_t b = 0;
    for (int c = 0; c < numcomp; c++) b += count[c] * (inputbuf[c].size() * sizeof(T) + obytes);
    return b;
  }

  // Compute<T>::report's table.
  void report() {
    std::vector<int> nc(CommBench::numproc), ni(CommBench::numproc);
    int numinput = 0;
    for (auto &v : inputbuf) numinput += (int)v.size();
    MPI_Allgather(&numcomp, 1, MPI_INT, nc.data(), 1, MPI_INT, CommBench::comm_mpi);
    MPI_Allgather(&numinput, 1, MPI_INT, ni.data(), 1, MPI_INT, CommBench::comm_mpi);
    if (CommBench::myid == CommBench::printid) {
      std::printf("numcomp: ");
      for (int p = 0; p < CommBench::numproc; p++) std::printf("%d(%d) ", nc[p], ni[p]);
      std::printf("\n\n");
    }
  }

  // Compute<T>::measure(warmup, numiter), pricing n * sizeof(T) + 4 bytes per
  // element (+ 8 when accumulating: bytes()), summed over ranks; the roofline line prices the busiest rank.
  void measure(int warmup, int numiter) {
    report();
    unsigned long busiest = (unsigned long)bytes(), tot = (unsigned long)bytes();
    MPI_Allreduce(MPI_IN_PLACE, &busiest, 1, MPI_UNSIGNED_LONG, MPI_MAX, CommBench::comm_mpi);
    MPI_Allreduce(MPI_IN_PLACE, &tot, 1, MPI_UNSIGNED_LONG, MPI_SUM, CommBench::comm_mpi);
    std::vector<double> times;
    if (CommBench::myid == CommBench::printid)
      std::printf("Measure Widened Reduction Kernel\n%d warmup iterations (in order)\n", warmup);
    for (int it = -warmup; it < numiter; it++) {
#ifndef HICCL_PORT_HOST
      CommBench::hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");
#endif
      MPI_Barrier(CommBench::comm_mpi);
      double t0 = MPI_Wtime();
      start();
      double st = MPI_Wtime() - t0;
      wait();
      double t = MPI_Wtime() - t0;
      MPI_Allreduce(MPI_IN_PLACE, &st, 1, MPI_DOUBLE, MPI_MAX, CommBench::comm_mpi);
      MPI_Allreduce(MPI_IN_PLACE, &t, 1, MPI_DOUBLE, MPI_MAX, CommBench::comm_mpi);
      if (it < 0) {
        if (CommBench::myid == CommBench::printid) std::printf("startup %.2e warmup: %e\n", st, t);
      } else {
        times.push_back(t);
      }
    }
    Compute<float>::roofline_bytes = (double)busiest;
    Compute<float>::print_times(times, (double)tot);
    Compute<float>::roofline_bytes = 0;
  }

 private:
  bool scaled = false;
  double scale = 1.0;
  bool accumulating = false;  // set_accumulate
  bool weighted = false;      // the first add decides
  std::vector<const float *> weightbuf;  // per compute: its weights, or NULL
#ifndef HICCL_PORT_HOST
  hiccl_reduce_plan_t *plan = nullptr;
  static void check(int e, const char *what) {
    if (e) CommBench::die(what, hiccl_last_error());
  }
#endif
};

}  // namespace HiCCL

#endif  // HICCL_COMPUTE_H
