// tests/cpp/avg_comm.cpp -- HiCCL::Comm<T>::set_scale end to end: the driver of
// tests/cpp/types_comm.cpp with an `alpha` argument, for the seven element types
// an averaging communicator takes.
//
//   mpirun -np P build/avg_comm_{hip,host} type counts patterns numstripe
//          ringnodes pipedepth hierarchy libs in_prefix out_prefix alpha
//
// Everything is types_comm's (see there), except:
//   * coll.set_scale(alpha) is called before the collective is composed, so
//     every REDUCE primitive of the composition carries the scale;
//   * pattern tokens: a number 1..8 with an optional suffix of letters that
//     mostly only goes into the file names (8o), and
//       r    one hand-made add_reduce of `count` elements from the ranks of
//            the OTHER ring node only (ranks np/ringnodes .. 2*np/ringnodes-1)
//            to rank 0: the receiver's node adds nothing, so the finished sum
//            is computed on the forwarding rank and only transferred;
//       a suffix c (8c)  clear_scale() follows set_scale(): the unscaled words;
//       x    two reduces under two different alphas: init() must die.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <string>
#include <vector>

#include "../../hiccl_amd/csrc/compose.h"

using namespace HiCCL;

static const size_t kGuard = 16;            // elements in front of and behind either buffer
static const unsigned char kPrefill = 0xA5;  // every byte of the receive allocation before a run

static std::vector<std::string> split(const std::string &t, char sep = ',') {
  std::vector<std::string> v;
  size_t p = 0;
  while (p <= t.size()) {
    size_t q = t.find(sep, p);
    if (q == std::string::npos) q = t.size();
    if (q > p) v.push_back(t.substr(p, q - p));
    p = q + 1;
  }
  return v;
}

static library lib_of(const std::string &w) {
  if (w == "ipc") return IPC;
  if (w == "ipc_get") return IPC_get;
  if (w == "mpi") return MPI;
  if (w == "xccl") return XCCL;
  CommBench::die("avg_comm", "unknown library " + w);
}

struct Args {
  std::vector<size_t> counts;
  std::vector<std::string> patterns;
  int numstripe, ringnodes, pipedepth;
  std::vector<int> hierarchy;
  std::vector<library> libs;
  std::string type, in_prefix, out_prefix;
  double alpha;
};

static std::string file_of(const std::string &prefix, const std::string &type, size_t count, const std::string &pattern) {
  return prefix + "." + type + "." + std::to_string(count) + ".p" + pattern + ".rank" + std::to_string(myid) + ".bin";
}

template <class T>
static int drive(const Args &a) {
  typedef unsigned char byte;
  const size_t cmax = *std::max_element(a.counts.begin(), a.counts.end());
  const size_t total = cmax * (size_t)numproc + 2 * kGuard;  // elements of either allocation
  T *sendall = nullptr, *recvall = nullptr;
  allocate(sendall, total);
  allocate(recvall, total);
  T *sendbuf = sendall + kGuard, *recvbuf = recvall + kGuard;
  const std::vector<byte> prefill(total * sizeof(T), kPrefill);
  std::vector<byte> host(total * sizeof(T));
  const char *rep = std::getenv("HICCL_DRIVER_REPEAT");
  const int repeat = rep && std::atoi(rep) > 1 ? std::atoi(rep) : 1;

  for (size_t count : a.counts)
    for (const std::string &token : a.patterns) {
      const size_t n = count * (size_t)numproc;
      std::fill(host.begin(), host.end(), (byte)0x5A);  // the send guards and the unused tail
      {
        const std::string path = file_of(a.in_prefix, a.type, count, token);
        FILE *f = std::fopen(path.c_str(), "rb");
        if (!f || std::fread(host.data() + kGuard * sizeof(T), sizeof(T), n, f) != n) CommBench::die("read", path);
        std::fclose(f);
      }
      CommBench::memcpyH2D((byte *)sendall, host.data(), host.size());
      {
        Comm<T> coll;
        coll.set_scale(a.alpha);
        if (token.find('c') != std::string::npos) coll.clear_scale();
        if (token == "r") {
          const int node = numproc / a.ringnodes;
          std::vector<int> senders;
          for (int p = node; p < 2 * node && p < numproc; p++) senders.push_back(p);
          coll.add_reduce(sendbuf, 0, recvbuf, 0, count, senders, 0);
        } else if (token == "x") {
          coll.add_reduction(sendbuf, recvbuf, count, all, 0);
          coll.set_scale(a.alpha * 2);
          coll.add_reduce(sendbuf, count, recvbuf, count, count, all, 0);
        } else {
          hiccl_driver::CommSink<T> sink{coll};
          if (!hiccl_driver::compose(sink, std::atoi(token.c_str()), sendbuf, recvbuf, count, numproc, 0))
            CommBench::die("avg_comm", "invalid pattern " + token);
        }
        coll.init(a.hierarchy, a.libs, a.numstripe, a.ringnodes, a.pipedepth);
        if (myid == 0 && count == a.counts.front()) coll.report();
        for (int r = 0; r < repeat; r++) {
          CommBench::memcpyH2D((byte *)recvall, prefill.data(), prefill.size());
          MPI_Barrier(comm_mpi);
          coll.start();
          coll.wait();
        }
        CommBench::memcpyD2H(host.data(), (const byte *)recvall, host.size());
        MPI_Barrier(comm_mpi);  // nobody frees schedule buffers a peer still reads
      }
      const std::string path = file_of(a.out_prefix, a.type, count, token);
      FILE *f = std::fopen(path.c_str(), "wb");
      if (!f || std::fwrite(host.data(), 1, host.size(), f) != host.size()) CommBench::die("write", path);
      std::fclose(f);
    }
  free(sendall);
  free(recvall);
  if (myid == 0)
    std::printf("avg_comm: %s: %zu collectives of %zu-byte elements done (%d ranks, %d run(s) each, alpha %.17g)\n",
                a.type.c_str(), a.counts.size() * a.patterns.size(), sizeof(T), numproc, repeat, a.alpha);
  return 0;
}

struct Entry {
  const char *name;
  int (*run)(const Args &);
};

// the types Comm<T>::set_scale takes
static const Entry kTypes[] = {
    {"bf16", drive<bf16>},
    {"f16", drive<f16>},
#ifdef __FLT16_MANT_DIG__
    {"_Float16", drive<_Float16>},
#endif
    {"f8e4m3", drive<f8e4m3>},
    {"f8e5m2", drive<f8e5m2>},
    {"double", drive<double>},
    {"float", drive<float>},
};

int main(int argc, char **argv) {
  CommBench::init();
  if (argc < 12) {
    if (myid == 0) {
      std::fprintf(stderr,
                   "usage: %s type counts patterns numstripe ringnodes pipedepth hierarchy libs in_prefix out_prefix "
                   "alpha\ntypes:",
                   argv[0]);
      for (const Entry &e : kTypes) std::fprintf(stderr, " %s", e.name);
      std::fprintf(stderr, "\n");
    }
    MPI_Finalize();
    return 2;
  }
  Args a;
  for (const std::string &w : split(argv[2])) a.counts.push_back((size_t)std::atol(w.c_str()));
  const std::vector<std::string> names = split(argv[1], '+'), lists = split(argv[3], '+');
  if (lists.size() != 1 && lists.size() != names.size()) CommBench::die("avg_comm", "one pattern list, or one per type");
  a.numstripe = std::atoi(argv[4]);
  a.ringnodes = std::atoi(argv[5]);
  a.pipedepth = std::atoi(argv[6]);
  for (const std::string &w : split(argv[7])) a.hierarchy.push_back(std::atoi(w.c_str()));
  for (const std::string &w : split(argv[8])) a.libs.push_back(lib_of(w));
  a.in_prefix = argv[9];
  a.out_prefix = argv[10];
  a.alpha = std::strtod(argv[11], nullptr);  // (17 significant digits round-trip a double)
  if (a.counts.empty() || names.empty()) CommBench::die("avg_comm", "no counts or no types");

  int rc = 0;
  for (size_t k = 0; k < names.size(); k++) {
    const std::string &name = names[k], &list = lists[lists.size() == 1 ? 0 : k];
    a.patterns = split(list);
    if (a.patterns.empty()) CommBench::die("avg_comm", "no patterns for " + name);
    const Entry *entry = nullptr;
    for (const Entry &e : kTypes)
      if (name == e.name) entry = &e;
    if (!entry) CommBench::die("avg_comm", "unknown type " + name);
    a.type = name;
    rc |= entry->run(a);
  }
  MPI_Finalize();
  return rc;
}
