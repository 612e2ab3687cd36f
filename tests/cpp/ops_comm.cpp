// tests/cpp/ops_comm.cpp -- HiCCL::Comm<maxof<float>>: a reduce to root 0
// under MPI, the program a user of the reference would write for a maximum.
//
//   mpirun -np P build/ops_comm_{hip,host} [count]
//
// Rank r sends count floats; the root receives their maximum.  The values are
// small integers with, per 17 elements, one NaN (on rank i mod P), one column
// of zeros of mixed sign (-0 on rank 0, +0 elsewhere: the maximum is +0), one
// column that is -0 on every rank (the maximum is -0, where a sum gives +0)
// and one -Inf / +Inf pair.  The root checks every element against the
// maximum it computes itself, a NaN by NaN-ness, the zeros by their sign bit.
// The source uses nothing but Comm<T> with T = maxof<float>: given ops.h's
// struct it compiles against the reference unchanged.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "hiccl.h"

using namespace HiCCL;

typedef maxof<float> T;

static float value_of(int rank, int ranks, size_t i) {
  switch (i % 17) {
    case 3: return (int)((i / 17) % ranks) == rank ? NAN : (float)rank;
    case 5: return rank == 0 ? -0.0f : 0.0f;
    case 7: return -0.0f;
    case 11: return rank == 0 ? -INFINITY : (rank == 1 ? INFINITY : 1.0f);
    default: return (float)((long)((i * 7 + (size_t)rank * 13) % 11) - 5);
  }
}

int main(int argc, char **argv) {
  CommBench::init();
  const size_t count = argc > 1 ? (size_t)std::atol(argv[1]) : 4099;
  T *sendbuf = nullptr;
  T *recvbuf = nullptr;
  allocate(sendbuf, count);
  allocate(recvbuf, count);
  unsigned long errors = 0;
  {
    Comm<T> reduce;
    reduce.add_reduction(sendbuf, recvbuf, count, HiCCL::all, 0);
    std::vector<int> hierarchy = {numproc};
    std::vector<library> lib = {IPC};
#ifdef HICCL_PORT_HOST
    lib = {MPI};
#endif
    reduce.init(hierarchy, lib, 1, 1, 1);

    std::vector<T> host(count);
    for (size_t i = 0; i < count; i++) host[i].v = value_of(myid, numproc, i);
    CommBench::memcpyH2D(sendbuf, host.data(), count);
    reduce.start();
    reduce.wait();

    if (myid == 0) {
      std::vector<T> out(count);
      CommBench::memcpyD2H(out.data(), recvbuf, count);
      for (size_t i = 0; i < count; i++) {
        T acc = 0;  // the reference's loop, on the host
        for (int r = 0; r < numproc; r++) {
          T x;
          x.v = value_of(r, numproc, i);
          acc += x;
        }
        uint32_t got, want;
        std::memcpy(&got, &out[i].v, 4);
        std::memcpy(&want, &acc.v, 4);
        const bool ok = std::isnan(acc.v) ? std::isnan(out[i].v) : got == want;
        if (!ok) {
          if (!errors) std::printf("first wrong element %zu: %#x, want %#x\n", i, got, want);
          errors++;
        }
      }
    }
  }
  MPI_Bcast(&errors, 1, MPI_UNSIGNED_LONG, 0, comm_mpi);
  if (myid == 0)
    std::printf("maxof<float> reduce to root: %s (%lu errors, %d ranks, count %zu)\n", errors ? "FAILED" : "PASSED", errors,
                numproc, count);
  free(sendbuf);
  free(recvbuf);
  MPI_Finalize();
  return errors ? 1 : 0;
}
