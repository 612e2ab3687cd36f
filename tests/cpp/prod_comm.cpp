// tests/cpp/prod_comm.cpp -- HiCCL::Comm<prodof<float>> and
// Comm<bxorof<uint64_t>>: reduces to root 0 under MPI, the programs a user of
// the reference would write for a product and for a checksum.
//
//   mpirun -np P build/prod_comm_{hip,host} [count]
//
// Rank r sends count elements; the root receives their product (float) and
// their exclusive-or (uint64_t).  The float contributions are powers of two
// and small integers, with a -0 on rank 0 per 17 elements, so the product is
// exact in any order and the expected word does not depend on the schedule; an
// exclusive-or never does.  The root checks every element against the fold it
// computes itself, bit for bit.  The source uses nothing but Comm<T> with the
// wrapper types: given ops.h's structs it compiles against the reference
// unchanged.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "hiccl.h"

using namespace HiCCL;

static void value_of(prodof<float> &x, int rank, size_t i) {
  static const float pow2[] = {0.125f, 0.5f, 1.0f, 2.0f, 16.0f, -4.0f, -0.25f};
  switch (i % 17) {
    case 3: x.v = rank == 0 ? -0.0f : 3.0f; break;
    case 5: x.v = (float)((long)((i + (size_t)rank) % 7) - 3) + ((i + (size_t)rank) % 7 == 3 ? 5.0f : 0.0f); break;
    default: x.v = pow2[(i * 5 + (size_t)rank * 3) % 7]; break;
  }
}

static void value_of(bxorof<uint64_t> &x, int rank, size_t i) {
  uint64_t z = (uint64_t)i * 0x9e3779b97f4a7c15ull + (uint64_t)(rank + 1) * 0xbf58476d1ce4e5b9ull;
  z ^= z >> 29;
  x.v = i % 17 == 7 ? ~(uint64_t)0 : z * 0x94d049bb133111ebull;
}

template <class T>
static unsigned long reduce_to_root(size_t count) {
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
    for (size_t i = 0; i < count; i++) value_of(host[i], myid, i);
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
          value_of(x, r, i);
          acc += x;
        }
        if (std::memcmp(&out[i].v, &acc.v, sizeof(acc.v)) != 0) {
          if (!errors) std::printf("first wrong element %zu\n", i);
          errors++;
        }
      }
    }
  }
  MPI_Bcast(&errors, 1, MPI_UNSIGNED_LONG, 0, comm_mpi);
  free(sendbuf);
  free(recvbuf);
  return errors;
}

int main(int argc, char **argv) {
  CommBench::init();
  const size_t count = argc > 1 ? (size_t)std::atol(argv[1]) : 4099;
  const unsigned long ep = reduce_to_root<prodof<float>>(count);
  const unsigned long ex = reduce_to_root<bxorof<uint64_t>>(count);
  if (myid == 0) {
    std::printf("prodof<float> reduce to root: %s (%lu errors, %d ranks, count %zu)\n", ep ? "FAILED" : "PASSED", ep,
                numproc, count);
    std::printf("bxorof<uint64_t> reduce to root: %s (%lu errors, %d ranks, count %zu)\n", ex ? "FAILED" : "PASSED", ex,
                numproc, count);
  }
  MPI_Finalize();
  return ep || ex ? 1 : 0;
}
