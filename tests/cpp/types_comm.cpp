// tests/cpp/types_comm.cpp -- HiCCL::Comm<T> end to end for every element type
// and operator wrapper: the eight collectives of compose.h on raw bytes.
//
//   mpirun -np P build/types_comm_{hip,host} type counts patterns numstripe
//          ringnodes pipedepth hierarchy libs in_prefix out_prefix
//
//   type      a name of the table below (bf16, maxof<f8e4m3>, ...), or several
//             joined by `+`, run one after the other
//   counts    comma list of elements per rank per chunk, e.g. 1,5,4099
//   patterns  comma list of 1 gather .. 8 allreduce, or `all`; a pattern may
//             carry a suffix of letters (8o) that only goes into the file
//             names, so that one launch runs a pattern on two sets of inputs;
//             with several types, one list for all or one per type joined by `+`
//   hierarchy comma list, e.g. 1,4,2;  libs: ipc|ipc_get|mpi|xccl per level
//
// The send and the receive buffer are allocated once, count_max * P elements
// with kGuard elements in front and behind.  For every (count, pattern) rank r
// reads its count * P send elements from <in_prefix>.<type>.<count>.p<pattern>.rank<r>.bin,
// fills the WHOLE receive allocation with the byte 0xA5, builds a fresh
// Comm<T>, composes the collective (root 0), init(hierarchy, libs, numstripe,
// ringnodes, pipedepth), start(), wait() -- HICCL_DRIVER_REPEAT=k: k times,
// the receive allocation refilled before each (graph mode: eager, capture +
// replay, replays) -- and writes the whole receive allocation, guards
// included, to <out_prefix>.<type>.<count>.p<pattern>.rank<r>.bin.
//
// The program knows nothing about values: bytes go in and out with memcpy,
// and the tests judge them (tests/comm_expected.py).
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
  CommBench::die("types_comm", "unknown library " + w);
}

struct Args {
  std::vector<size_t> counts;
  std::vector<std::string> patterns;  // the id, then an optional suffix for the file names
  int numstripe, ringnodes, pipedepth;
  std::vector<int> hierarchy;
  std::vector<library> libs;
  std::string type, in_prefix, out_prefix;
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
      const int pattern = std::atoi(token.c_str());
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
        hiccl_driver::CommSink<T> sink{coll};
        if (!hiccl_driver::compose(sink, pattern, sendbuf, recvbuf, count, numproc, 0))
          CommBench::die("types_comm", "invalid pattern " + token);
        coll.init(a.hierarchy, a.libs, a.numstripe, a.ringnodes, a.pipedepth);
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
    std::printf("types_comm: %s: %zu collectives of %zu-byte elements done (%d ranks, %d run(s) each)\n", a.type.c_str(),
                a.counts.size() * a.patterns.size(), sizeof(T), numproc, repeat);
  return 0;
}

struct Entry {
  const char *name;
  int (*run)(const Args &);
};

// SUM types, then the operator wrappers (include/hiccl/ops.h)
static const Entry kTypes[] = {
    {"bf16", drive<bf16>},
    {"f16", drive<f16>},
    {"f8e4m3", drive<f8e4m3>},
    {"f8e5m2", drive<f8e5m2>},
    {"int32_t", drive<int32_t>},
    {"double", drive<double>},
    {"float", drive<float>},
    {"size_t", drive<size_t>},
    {"maxof<bf16>", drive<maxof<bf16>>},
    {"minof<f16>", drive<minof<f16>>},
    {"maxof<f8e4m3>", drive<maxof<f8e4m3>>},
    {"minof<f8e5m2>", drive<minof<f8e5m2>>},
    {"maxof<int32_t>", drive<maxof<int32_t>>},
    {"minof<double>", drive<minof<double>>},
    {"prodof<bf16>", drive<prodof<bf16>>},
    {"prodof<f16>", drive<prodof<f16>>},
    {"bandof<int32_t>", drive<bandof<int32_t>>},
    {"borof<uint64_t>", drive<borof<uint64_t>>},
};

int main(int argc, char **argv) {
  CommBench::init();
  if (argc < 11) {
    if (myid == 0) {
      std::fprintf(stderr,
                   "usage: %s type counts patterns numstripe ringnodes pipedepth hierarchy libs in_prefix out_prefix\ntypes:",
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
  if (lists.size() != 1 && lists.size() != names.size()) CommBench::die("types_comm", "one pattern list, or one per type");
  a.numstripe = std::atoi(argv[4]);
  a.ringnodes = std::atoi(argv[5]);
  a.pipedepth = std::atoi(argv[6]);
  for (const std::string &w : split(argv[7])) a.hierarchy.push_back(std::atoi(w.c_str()));
  for (const std::string &w : split(argv[8])) a.libs.push_back(lib_of(w));
  a.in_prefix = argv[9];
  a.out_prefix = argv[10];
  if (a.counts.empty() || names.empty()) CommBench::die("types_comm", "no counts or no types");

  int rc = 0;
  for (size_t k = 0; k < names.size(); k++) {
    const std::string &name = names[k], &list = lists[lists.size() == 1 ? 0 : k];
    a.patterns.clear();
    if (list == "all")
      for (int p = gather; p <= allreduce; p++) a.patterns.push_back(std::to_string(p));
    else
      a.patterns = split(list);
    if (a.patterns.empty()) CommBench::die("types_comm", "no patterns for " + name);
    const Entry *entry = nullptr;
    for (const Entry &e : kTypes)
      if (name == e.name) entry = &e;
    if (!entry) CommBench::die("types_comm", "unknown type " + name);
    a.type = name;
    rc |= entry->run(a);
  }
  MPI_Finalize();
  return rc;
}
