// include/hiccl/transport.h -- point-to-point transport under HiCCL's schedule.
//
// The reference builds on the CommBench submodule, which is not vendored
// (/root/reference/.gitmodules:1-3, empty CommBench/).  This header provides
// the names HiCCL and collectives/main.cpp call (call sites: SURVEY.md
// section 1, L0 row) with an MI355X-native implementation:
//
//   control plane  MPI (rank/size, handle exchange, completion tokens)
//   IPC / IPC_get  HIP IPC over xGMI: device allocations exported with
//                  hipIpcGetMemHandle, opened once per peer allocation,
//                  moved by one batched copy kernel per step (a HICCL_BYTES
//                  plan) of the writer (IPC, "put") or the reader (IPC_get,
//                  "get"); ready/done tokens (MPI messages, or device flags
//                  in stream-ordered mode) keep a step from overwriting
//                  bytes a peer still reads
//   MPI            MPI_Isend/Irecv; device buffers staged through pinned
//                  host memory (MPICH here is not GPU-aware)
//   XCCL           RCCL point-to-point (ncclSend/ncclRecv in one group per
//                  step on the transport stream) when built with
//                  HICCL_WITH_RCCL, asked for with HICCL_XCCL=rccl, and
//                  every rank drives its own GPU (RCCL refuses two ranks on
//                  one device); otherwise the level runs on the IPC path and
//                  init() says so
//   dummy          nothing
//
// Host port (HICCL_PORT_HOST, config 1: no GPU): buffers are host memory and
// every library moves data with MPI.
#ifndef HICCL_TRANSPORT_H
#define HICCL_TRANSPORT_H

// The deprecated MPI C++ bindings would declare a namespace MPI that
// collides with the library name MPI used unqualified (README.md:46).
#ifndef MPICH_SKIP_MPICXX
#define MPICH_SKIP_MPICXX 1
#endif
#ifndef OMPI_SKIP_MPICXX
#define OMPI_SKIP_MPICXX 1
#endif
#include <mpi.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <string>
#include <vector>

#ifndef HICCL_PORT_HOST
#include <hip/hip_runtime_api.h>

#include "../hiccl_reduce.h"
#ifdef HICCL_WITH_RCCL
#include <rccl/rccl.h>
#endif
#endif

#include <unistd.h>

namespace CommBench {

enum library { dummy, IPC, IPC_get, MPI, XCCL, numlib };

inline MPI_Comm comm_mpi = MPI_COMM_NULL;
inline int printid = 0;
inline int myid = 0;
inline int numproc = 1;
inline int mydevice = 0;
inline size_t memory = 0;  // bytes allocated through allocate()
// Stream-ordered mode (HIP port, every rank on one node): transfers and
// their synchronisation are enqueued on the rank's stream, no host round
// trip per step.  Set by HiCCL::Comm::init before it builds the transports.
inline bool stream_ordered = false;

[[noreturn]] inline void die(const char *what, const std::string &msg) {
  std::fprintf(stderr, "[hiccl rank %d] %s: %s\n", myid, what, msg.c_str());
  std::fflush(stderr);
  int init = 0;
  MPI_Initialized(&init);
  if (init) MPI_Abort(MPI_COMM_WORLD, 1);
  std::abort();
}

#ifndef HICCL_PORT_HOST
inline void hip_check(hipError_t e, const char *what) {
  if (e != hipSuccess) die(what, hipGetErrorString(e));
}
#endif

inline void mpi_check(int e, const char *what) {
  if (e != MPI_SUCCESS) die(what, "MPI error " + std::to_string(e));
}

// Bind this thread to the rank's device (reference: setup_gpu before run()
// on the Comm::start pthread, comm.h:214-216).
inline void setup_gpu() {
#ifndef HICCL_PORT_HOST
  hip_check(hipSetDevice(mydevice), "hipSetDevice");
#endif
}

// MPI bootstrap; one device per local rank (round-robin over visible GPUs).
inline void init() {
  int flag = 0;
  MPI_Initialized(&flag);
  if (!flag) {
    int provided = 0;
    MPI_Init_thread(nullptr, nullptr, MPI_THREAD_SERIALIZED, &provided);
  }
  if (comm_mpi == MPI_COMM_NULL) MPI_Comm_dup(MPI_COMM_WORLD, &comm_mpi);
  MPI_Comm_rank(comm_mpi, &myid);
  MPI_Comm_size(comm_mpi, &numproc);
#ifndef HICCL_PORT_HOST
  MPI_Comm local;
  MPI_Comm_split_type(comm_mpi, MPI_COMM_TYPE_SHARED, myid, MPI_INFO_NULL, &local);
  int lrank = 0;
  MPI_Comm_rank(local, &lrank);
  MPI_Comm_free(&local);
  int ndev = 0;
  hip_check(hipGetDeviceCount(&ndev), "hipGetDeviceCount");
  if (ndev < 1) die("init", "no HIP device");
  mydevice = lrank % ndev;
  setup_gpu();
  // HICCL_SYNC=spin|yield|blocking: how host synchronisations wait (HIP's
  // default is auto); host-driven steps synchronise twice per step
  if (const char *m = std::getenv("HICCL_SYNC")) {
    const std::string v = m;
    const unsigned f = v == "spin" ? hipDeviceScheduleSpin : v == "yield" ? hipDeviceScheduleYield
                       : v == "blocking" ? hipDeviceScheduleBlockingSync : hipDeviceScheduleAuto;
    if (hipSetDeviceFlags(f) != hipSuccess) (void)hipGetLastError();
  }
#endif
}

#ifndef HICCL_PORT_HOST
// True on every rank when two or more ranks of comm_mpi drive the same
// device (same host, same PCI bus id): CommBench::init assigns devices
// round-robin, so a node with more ranks than GPUs shares them.
// Collective over comm_mpi.
// Every rank's "host/PCI bus id" (collective over comm_mpi).
inline std::vector<std::string> device_keys() {
  char key[192];
  std::memset(key, 0, sizeof(key));
  char host[96] = {0};
  (void)gethostname(host, sizeof(host) - 1);
  char bus[64] = {0};
  hip_check(hipDeviceGetPCIBusId(bus, sizeof(bus) - 1, mydevice), "hipDeviceGetPCIBusId");
  std::snprintf(key, sizeof(key), "%s/%s", host, bus);
  std::vector<char> all((size_t)numproc * sizeof(key));
  mpi_check(MPI_Allgather(key, sizeof(key), MPI_CHAR, all.data(), sizeof(key), MPI_CHAR, comm_mpi),
            "MPI_Allgather(device keys)");
  std::vector<std::string> keys;
  for (int r = 0; r < numproc; r++) keys.emplace_back(all.data() + (size_t)r * sizeof(key));
  return keys;
}
inline bool ranks_share_device() {
  std::vector<std::string> keys = device_keys();
  std::sort(keys.begin(), keys.end());
  return std::adjacent_find(keys.begin(), keys.end()) != keys.end();
}
// Ranks (this one included) driving this rank's device.  Collective.
inline int ranks_on_my_device() {
  const std::vector<std::string> keys = device_keys();
  return (int)std::count(keys.begin(), keys.end(), keys[myid]);
}

// ------------------------------------------------------------- RCCL ------
// The XCCL library level: one RCCL communicator over comm_mpi, created by
// xccl_setup() (collective) before any Comm<T> of an XCCL level is built.
inline bool &xccl_on() {
  static bool on = false;
  return on;
}
#ifdef HICCL_WITH_RCCL
inline ncclComm_t &xccl_comm() {
  static ncclComm_t c = nullptr;
  return c;
}
inline void nccl_check(ncclResult_t e, const char *what) {
  if (e != ncclSuccess) die(what, ncclGetErrorString(e));
}
#endif
// HICCL_XCCL=rccl opts the XCCL levels into RCCL.  Until a run with one GPU
// per rank has passed the known-answer test the RCCL path is not the
// default: XCCL levels take the (tested) xGMI IPC path unless asked.
inline bool xccl_rccl_requested() {
  const char *e = std::getenv("HICCL_XCCL");
  return e && std::string(e) == "rccl";
}
// HICCL_XCCL_SELF=rccl (test knob): a rank's self transfers of an XCCL level
// go through RCCL too (ncclSend / ncclRecv to itself in the step's group)
// instead of the batched copy kernel -- so a one-rank job on one GPU runs
// the RCCL path end to end (communicator, groups, destroy) and the KAT
// checks the bytes RCCL moved.  RCCL refuses two ranks on one GPU, so this
// is the only form of the path a single-GPU box can execute.
inline bool xccl_self_on_rccl() {
  const char *e = std::getenv("HICCL_XCCL_SELF");
  return e && std::string(e) == "rccl";
}

// Communicators whose XCCL levels run on RCCL; the last one to go destroys
// the RCCL communicator (xccl_release), so ncclCommDestroy runs before
// MPI_Finalize in every driver that scopes its HiCCL::Comm.
inline int &xccl_users() {
  static int n = 0;
  return n;
}

// Collective.  Returns whether XCCL levels run on RCCL; otherwise they run
// on the IPC path (not requested, no RCCL in this build, or ranks sharing a
// device).  A true return must be paired with xccl_release().
inline bool xccl_setup(bool shared_device) {
#ifdef HICCL_WITH_RCCL
  if (!xccl_rccl_requested()) return false;
  if (xccl_on()) {
    xccl_users()++;
    return true;
  }
  if (shared_device) return false;
  ncclUniqueId id;
  if (myid == 0) nccl_check(ncclGetUniqueId(&id), "ncclGetUniqueId");
  mpi_check(MPI_Bcast(&id, sizeof(id), MPI_BYTE, 0, comm_mpi), "MPI_Bcast(nccl id)");
  setup_gpu();
  nccl_check(ncclCommInitRank(&xccl_comm(), numproc, id, myid), "ncclCommInitRank");
  xccl_on() = true;
  xccl_users() = 1;
  return true;
#else
  (void)shared_device;
  return false;
#endif
}

// Drop one user of the RCCL communicator; the last destroys it (after the
// caller has synchronised every stream RCCL work was enqueued on).
inline void xccl_release() {
#ifdef HICCL_WITH_RCCL
  if (!xccl_on() || --xccl_users() > 0) return;
  setup_gpu();
  (void)ncclCommDestroy(xccl_comm());
  xccl_comm() = nullptr;
  xccl_on() = false;
#endif
}

// One transport stream per process: the steps of a pipeline run one after
// the other on a rank, so every Comm shares it (the reference creates
// streams per object; hundreds of them oversubscribe the hardware queues).
inline hipStream_t transport_stream() {
  static hipStream_t s = [] {
    hipStream_t t;
    hip_check(hipStreamCreateWithFlags(&t, hipStreamNonBlocking), "hipStreamCreate(transport)");
    return t;
  }();
  return s;
}
#endif

inline void print_data(size_t bytes) {
  if (bytes < 1e3) std::printf("%d bytes", (int)bytes);
  else if (bytes < 1e6) std::printf("%.4f KB", bytes / 1e3);
  else if (bytes < 1e9) std::printf("%.4f MB", bytes / 1e6);
  else std::printf("%.4f GB", bytes / 1e9);
}

inline const char *lib_name(library lib) {
  switch (lib) {
    case dummy: return "dummy";
    case IPC: return "IPC";
    case IPC_get: return "IPC_get";
    case MPI: return "MPI";
    case XCCL: return "XCCL";
    default: return "numlib";
  }
}

inline void print_lib(library lib) { std::printf("%s", lib_name(lib)); }

#ifndef HICCL_PORT_HOST
inline size_t &ipc_retired_bytes();
inline size_t ipc_retired_max();
#endif

// Collective.  Bytes allocated through allocate() over all ranks, and (HIP
// port) the peers' freed allocations this process's retired IPC mappings
// still keep alive (see IpcMapping) with their cap, largest rank.
inline void report_memory() {
  size_t mine[3] = {memory, 0, 0};
#ifndef HICCL_PORT_HOST
  mine[1] = ipc_retired_bytes();
  mine[2] = ipc_retired_max();
#endif
  std::vector<size_t> all((size_t)numproc * 3);
  MPI_Allgather(mine, sizeof(mine), MPI_BYTE, all.data(), sizeof(mine), MPI_BYTE, comm_mpi);
  if (myid == printid) {
    size_t tot = 0, ret = 0, cap = 0;
    for (int p = 0; p < numproc; p++) {
      tot += all[3 * p];
      ret = std::max(ret, all[3 * p + 1]);
      cap = std::max(cap, all[3 * p + 2]);
    }
    std::printf("CommBench memory: ");
    print_data(tot);
    std::printf(" total over %d ranks", numproc);
#ifndef HICCL_PORT_HOST
    std::printf("; retired IPC mappings keep ");
    print_data(ret);
    std::printf(" of peer memory alive (largest rank; cap ");
    print_data(cap);
    std::printf(")");
#endif
    std::printf("\n");
  }
}

// ------------------------------------------------------------- memory ----

template <typename T>
void allocate(T *&p, size_t n) {
  const size_t bytes = std::max<size_t>(n, 1) * sizeof(T);
#ifdef HICCL_PORT_HOST
  p = static_cast<T *>(std::malloc(bytes));
  if (!p) die("allocate", "malloc failed");
#else
  hip_check(hipMalloc((void **)&p, bytes), "hipMalloc");
#endif
  memory += bytes;
}

template <typename T>
void free(T *p) {
  if (!p) return;
#ifdef HICCL_PORT_HOST
  std::free(p);
#else
  hip_check(hipFree(p), "hipFree");
#endif
}

template <typename T>
void memcpyH2D(T *d, const T *s, size_t n) {
#ifdef HICCL_PORT_HOST
  std::memcpy(d, s, n * sizeof(T));
#else
  hip_check(hipMemcpy(d, s, n * sizeof(T), hipMemcpyHostToDevice), "memcpyH2D");
#endif
}

template <typename T>
void memcpyD2H(T *d, const T *s, size_t n) {
#ifdef HICCL_PORT_HOST
  std::memcpy(d, s, n * sizeof(T));
#else
  hip_check(hipMemcpy(d, s, n * sizeof(T), hipMemcpyDeviceToHost), "memcpyD2H");
#endif
}

template <typename T>
void memcpyD2D(T *d, const T *s, size_t n) {
#ifdef HICCL_PORT_HOST
  std::memmove(d, s, n * sizeof(T));
#else
  hip_check(hipMemcpy(d, s, n * sizeof(T), hipMemcpyDeviceToDevice), "memcpyD2D");
#endif
}

#ifndef HICCL_PORT_HOST
// ------------------------------------------------------- IPC registry ----
// One open mapping per (peer rank, peer allocation base).
struct IpcKey {
  int rank;
  uintptr_t base;
  bool operator<(const IpcKey &o) const { return rank != o.rank ? rank < o.rank : base < o.base; }
};

struct IpcExport {
  hipIpcMemHandle_t handle;
  uint64_t base;    // peer's allocation base (identifies the mapping)
  uint64_t offset;  // byte offset of the buffer inside that allocation
  uint64_t size;    // bytes of that allocation
  uint64_t nonce;   // probe value written at the buffer (probe != 0), see ipc_probe_*
  uint32_t probe;   // bytes of the probe (0: no probe)
  uint32_t recycled;  // the base was exported before for another allocation
};

// Mappings are reference-counted per holder (a transport, a flag space).
// When the last holder lets go, the mapping is RETIRED, not closed: on ROCm
// 7.2 (dmabuf IPC) closing a mapping and later opening a peer's NEW
// allocation that the peer's allocator placed at a freed exported address
// yields a mapping that reaches other memory -- writes through it are lost
// (measured: 4 ranks x 5 recreated communicators on reallocated buffers fail
// within 1-3 runs when mappings are closed, never when they stay open; a
// 200 ms pause after the close does not help; tests/test_mpi_gpu.py
// ::test_recreated_communicators_on_reallocated_buffers; the two-process
// reproducer tests/cpp/ipc_reuse.cpp, tests/test_ipc_reuse_gpu.py).  A
// retired mapping is revived when the peer exports the same allocation
// again (same base, not recycled) and closed, oldest first, only when the
// retired mappings exceed the cap or on ipc_trim().  The cap
// (HICCL_IPC_RETIRED_MAX bytes) is tied to what this process maps
// (ipc_retired_max): a bounded number of generations of its peers' buffers
// stay alive after they are freed, never more than a quarter of HBM.  A mapping opened for a recycled address is
// verified by a probe (ipc_probe_*), so a closed-then-reopened address that
// misses fails loudly instead of losing data.
struct IpcMapping {
  char *ptr;
  int refs;
  size_t bytes;  // of the mapped allocation
};

inline std::map<IpcKey, IpcMapping> &ipc_opened() {
  static std::map<IpcKey, IpcMapping> m;
  return m;
}

struct IpcRetired {
  IpcKey key;
  char *ptr;
  size_t bytes;
};
inline std::vector<IpcRetired> &ipc_retired() {  // oldest first
  static std::vector<IpcRetired> r;
  return r;
}
inline size_t &ipc_retired_bytes() {
  static size_t b = 0;
  return b;
}
// Bytes of peer allocations mapped (live, not retired) right now, and the
// most there ever were at once.
inline size_t &ipc_live_bytes() {
  static size_t b = 0;
  return b;
}
inline size_t &ipc_live_peak() {
  static size_t b = 0;
  return b;
}
// Default cap: kIpcRetiredGenerations x the most peer memory this process
// has had mapped at once, at least 256 MiB, at most a quarter of the
// device's memory.  Measured (round 3): at 2 x, the 4-rank test that
// recreates communicators on freshly allocated buffers every round
// (test_recreated_communicators_on_reallocated_buffers) was stopped by the
// recycled-address probe in round 3 of 5 -- closes the cap forces meet the
// runtime behaviour the retirement avoids -- so the cap keeps many
// generations; a job that outgrows it is stopped by the probe, never
// silently wrong.
constexpr size_t kIpcRetiredGenerations = 16;
inline size_t ipc_retired_max() {
  static const long long env = [] {
    const char *e = std::getenv("HICCL_IPC_RETIRED_MAX");
    return e ? (long long)std::strtoull(e, nullptr, 0) : -1ll;
  }();
  if (env >= 0) return (size_t)env;
  static const size_t ceiling = [] {
    size_t fr = 0, total = 0;
    if (hipMemGetInfo(&fr, &total) != hipSuccess) {
      (void)hipGetLastError();
      return (size_t)16 << 30;
    }
    return total / 4;
  }();
  const size_t want = std::max(kIpcRetiredGenerations * ipc_live_peak(), (size_t)256 << 20);
  return std::min(want, ceiling);
}

// HICCL_DEBUG_IPC=1: every export, import and close on stdout; =2: kept in
// memory (timing barely changes) and printed by ipc_log_dump().
inline int ipc_debug() {
  static const int on = [] {
    const char *e = std::getenv("HICCL_DEBUG_IPC");
    return e ? std::atoi(e) : 0;
  }();
  return on;
}
inline std::string &ipc_log() {
  static std::string s;
  return s;
}
template <typename... A>
void ipc_note(const char *fmt, A... a) {
  char line[256];
  std::snprintf(line, sizeof(line), fmt, a...);
  if (ipc_debug() == 1) std::fputs(line, stdout);
  else ipc_log() += line;
}
inline void ipc_log_dump() {
  std::fputs(ipc_log().c_str(), stdout);
  std::fflush(stdout);
}
inline std::string handle_hex(const hipIpcMemHandle_t &h) {  // the handle's bytes as 32-bit words
  const uint32_t *w = reinterpret_cast<const uint32_t *>(&h);
  std::string s;
  char b[12];
  for (size_t i = 0; i < sizeof(h) / 4; i++) {
    std::snprintf(b, sizeof(b), "%s%x", i ? "." : "", w[i]);
    s += b;
  }
  return s;
}
inline unsigned long long handle_hash(const hipIpcMemHandle_t &h) {  // FNV-1a of the handle bytes
  const unsigned char *b = reinterpret_cast<const unsigned char *>(&h);
  unsigned long long x = 1469598103934665603ull;
  for (size_t i = 0; i < sizeof(h); i++) x = (x ^ b[i]) * 1099511628211ull;
  return x;
}

// Allocation ids (HIP's unique buffer id per allocation) of the bases this
// process has exported, per importing rank: a base exported again to that
// rank for a DIFFERENT allocation is a recycled address (an exported buffer
// was freed and the allocator handed its address back), which the importer
// must neither revive its retired mapping for nor trust unverified.
inline std::map<std::pair<uintptr_t, int>, unsigned long long> &ipc_exported_ids() {
  static std::map<std::pair<uintptr_t, int>, unsigned long long> m;
  return m;
}

// `to`: the importing rank, or -1 for every other rank (a flag space).
inline IpcExport ipc_export(const void *p, int to) {
  IpcExport e;
  std::memset(&e, 0, sizeof(e));
  hipDeviceptr_t base = nullptr;
  size_t size = 0;
  hip_check(hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)p), "hipMemGetAddressRange");
  hip_check(hipIpcGetMemHandle(&e.handle, (void *)base), "hipIpcGetMemHandle");
  e.base = (uint64_t)(uintptr_t)base;
  e.offset = (uint64_t)((const char *)p - (const char *)base);
  e.size = (uint64_t)size;
  unsigned long long id = 0;
  if (hipPointerGetAttribute(&id, HIP_POINTER_ATTRIBUTE_BUFFER_ID, base) != hipSuccess) {
    (void)hipGetLastError();
    e.recycled = 1;  // unknown: never revive, verify
  } else {
    auto &ids = ipc_exported_ids();
    for (int r = 0; r < numproc; r++) {
      if (r == myid || (to >= 0 && r != to)) continue;
      auto it = ids.find({(uintptr_t)base, r});
      if (it != ids.end() && it->second != id) e.recycled = 1;
      ids[{(uintptr_t)base, r}] = id;
    }
  }
  if (ipc_debug())
    ipc_note("[ipc %d] export %p = base %p + %llu (size %zu)%s handle %016llx [%s]\n", myid, p, (void *)base,
             (unsigned long long)e.offset, size, e.recycled ? " recycled" : "", handle_hash(e.handle),
             handle_hex(e.handle).c_str());
  return e;
}

// Probe of a mapping of a recycled base (owner side, before the export is
// sent): save the first `bytes` (<= 8) of the buffer, write a nonce there.
// The mover reads them through its mapping (ipc_probe_check) and answers;
// ipc_probe_finish restores the bytes (see IpcMapping for why).
inline uint64_t ipc_probe_begin(IpcExport &e, void *p, size_t bytes) {
  static uint64_t counter = 0x9e3779b97f4a7c15ull;
  uint64_t saved = 0;
  e.probe = (uint32_t)std::min<size_t>(bytes, 8);
  if (!e.probe) return 0;
  // the null-stream copies below are not ordered with the caller's
  // non-blocking streams: let a producer still writing the buffer finish
  // first, so the saved bytes are the ones the restore must put back
  hip_check(hipDeviceSynchronize(), "probe: drain the device");
  hip_check(hipMemcpy(&saved, p, e.probe, hipMemcpyDeviceToHost), "probe save");
  counter = counter * 6364136223846793005ull + 1442695040888963407ull + (uint64_t)myid;
  e.nonce = counter ^ saved;  // never the current contents
  if (std::memcmp(&e.nonce, &saved, e.probe) == 0) e.nonce = ~saved;
  hip_check(hipMemcpy(p, &e.nonce, e.probe, hipMemcpyHostToDevice), "probe write");
  return saved;
}
// 0: both views see the nonce; bit 0: the copy engine's view differs; bit 1:
// a kernel's view (what the transfers use) differs.  `room`: bytes from
// `mapped` to the end of the mapping as the runtime records it; hipMemcpy
// refuses a read past that ("invalid argument"), so where the record is
// shorter than the probe (ipc_import: a mapping kept from a smaller buffer)
// the kernel's view, the one the transfers use, is the one checked.
inline int ipc_probe_check(const IpcExport &e, const void *mapped, size_t room, std::string *seen = nullptr) {
  uint64_t got = e.nonce, got_k = 0;
  if (room >= e.probe) hip_check(hipMemcpy(&got, mapped, e.probe, hipMemcpyDeviceToHost), "probe read");
  static uint64_t *scratch = nullptr;
  if (!scratch) hip_check(hipMalloc((void **)&scratch, 64), "probe scratch");
  if (hiccl_stream_copy(scratch, mapped, e.probe, nullptr)) die("probe", hiccl_last_error());
  hip_check(hipDeviceSynchronize(), "probe sync");
  hip_check(hipMemcpy(&got_k, scratch, e.probe, hipMemcpyDeviceToHost), "probe read (kernel)");
  if (seen) {
    char b[160];
    std::snprintf(b, sizeof(b), "nonce %016llx, copy engine %016llx, kernel %016llx", (unsigned long long)e.nonce,
                  (unsigned long long)got, (unsigned long long)got_k);
    *seen = b;
  }
  return (std::memcmp(&got, &e.nonce, e.probe) != 0) | (std::memcmp(&got_k, &e.nonce, e.probe) != 0) << 1;
}
inline void ipc_probe_finish(const IpcExport &e, void *p, uint64_t saved) {
  hip_check(hipMemcpy(p, &saved, e.probe, hipMemcpyHostToDevice), "probe restore");
}

inline void ipc_close_oldest_retired() {
  auto &r = ipc_retired();
  if (r.empty()) return;
  if (ipc_debug())
    ipc_note("[ipc %d] close retired peer %d base %#llx at %p\n", myid, r.front().key.rank,
             (unsigned long long)r.front().key.base, (void *)r.front().ptr);
  (void)hipIpcCloseMemHandle(r.front().ptr);
  ipc_retired_bytes() -= r.front().bytes;
  r.erase(r.begin());
}

// Close every retired mapping (the peers' freed allocations they keep alive
// are released).  Safe whenever no communicator is being created.
inline void ipc_trim() {
  while (!ipc_retired().empty()) ipc_close_oldest_retired();
}

// Bytes of the allocation mapped at `ptr` as the runtime knows it (0: unknown).
inline size_t ipc_mapped_bytes(void *ptr) {
  hipDeviceptr_t mb = nullptr;
  size_t bytes = 0;
  if (hipMemGetAddressRange(&mb, &bytes, (hipDeviceptr_t)ptr) != hipSuccess) {
    (void)hipGetLastError();
    bytes = 0;
  }
  return bytes;
}

// The mapping of peer's exported buffer; its key is appended to `held`,
// which the holder hands to ipc_release when it no longer uses the mapping.
inline char *ipc_import(int peer, const IpcExport &e, std::vector<IpcKey> &held) {
  IpcKey k{peer, (uintptr_t)e.base};
  auto &m = ipc_opened();
  auto it = m.find(k);
  if (it == m.end()) {
    auto &r = ipc_retired();
    auto rit = r.end();
    for (auto i = r.begin(); i != r.end(); ++i)  // the most recent retired mapping of this base
      if (i->key.rank == k.rank && i->key.base == k.base) rit = i;
    if (rit != r.end() && !e.recycled) {  // the same allocation as when it was retired: revive
      it = m.emplace(k, IpcMapping{rit->ptr, 0, rit->bytes}).first;
      ipc_retired_bytes() -= rit->bytes;
      r.erase(rit);
      ipc_live_bytes() += it->second.bytes;
    } else {
      void *ptr = nullptr;
      hip_check(hipIpcOpenMemHandle(&ptr, e.handle, hipIpcMemLazyEnablePeerAccess), "hipIpcOpenMemHandle");
      size_t bytes = ipc_mapped_bytes(ptr);
      if (bytes && bytes < e.size) {
        // The peer freed a small buffer and allocated a LARGER one at its
        // address (communicators over buffers of growing sizes: a 4-byte
        // stage buffer, then one of 2734 bytes).  Small allocations are
        // fragments of one block of the peer's allocator, a mapping is of the
        // whole block, and while the retired mapping of the freed fragment is
        // open the runtime resolves the new handle to it: the same pointer,
        // recorded at the OLD size.  The memory is reached (the probe of this
        // recycled export verifies it with a kernel); only the runtime's
        // record is short, so host copies past it are refused
        // (ipc_probe_check).  Closing the retired mappings and opening the
        // handle again is no way out: it fails now and then on ROCm 7.2
        // ("hipIpcOpenMemHandle: invalid device pointer", the behaviour the
        // retirement exists for).  Any other short mapping stops the job
        // before a kernel runs past it.
        bool kept = false;
        for (const IpcRetired &old : r) kept = kept || (old.key.rank == k.rank && old.key.base == k.base && old.ptr == ptr);
        if (ipc_debug())
          ipc_note("[ipc %d] peer %d base %#llx: mapping recorded at %zu B for an allocation of %llu B%s\n", myid, peer,
                   (unsigned long long)e.base, bytes, (unsigned long long)e.size, kept ? " (a retired mapping's)" : "");
        if (!kept || !e.recycled)
          die("transport", "the IPC mapping of rank " + std::to_string(peer) + "'s buffer covers " + std::to_string(bytes) +
                           " of its " + std::to_string(e.size) + " bytes");
      }
      it = m.emplace(k, IpcMapping{(char *)ptr, 0, bytes}).first;
      ipc_live_bytes() += bytes;
    }
    ipc_live_peak() = std::max(ipc_live_peak(), ipc_live_bytes());
  }
  it->second.refs++;
  held.push_back(k);
  if (ipc_debug())
    ipc_note("[ipc %d] import peer %d base %#llx + %llu -> %p (refs %d) handle %016llx\n", myid, peer,
             (unsigned long long)e.base, (unsigned long long)e.offset, (void *)(it->second.ptr + e.offset),
             it->second.refs, handle_hash(e.handle));
  return it->second.ptr + e.offset;
}

inline void ipc_release(std::vector<IpcKey> &held) {
  auto &m = ipc_opened();
  for (const IpcKey &k : held) {
    auto it = m.find(k);
    if (it == m.end()) continue;
    if (--it->second.refs == 0) {
      if (ipc_debug())
        ipc_note("[ipc %d] retire peer %d base %#llx at %p\n", myid, k.rank, (unsigned long long)k.base,
                 (void *)it->second.ptr);
      ipc_retired().push_back(IpcRetired{k, it->second.ptr, it->second.bytes});
      ipc_retired_bytes() += it->second.bytes;
      ipc_live_bytes() -= it->second.bytes;
      m.erase(it);
    }
  }
  held.clear();
  while (!ipc_retired().empty() && ipc_retired_bytes() > ipc_retired_max()) ipc_close_oldest_retired();
}

// A communicator's flag array: one uint32 per slot in device memory on every
// rank, IPC-mapped by every other rank (flags of peers are written remotely
// with system-scope release stores, local flags polled with acquire loads by
// hiccl_signal_wait).  err is host-visible and set by a timed-out spin.
struct FlagSpace {
  uint32_t *local = nullptr;
  std::vector<uint32_t *> peer;  // peer[r]: rank r's array as mapped here (peer[myid] = local)
  size_t nflags = 0;
  uint32_t *err = nullptr;
  std::vector<IpcKey> held;  // peers' flag arrays mapped here

  // Collective over comm_mpi.
  // The flags are uncached device memory (hipDeviceMallocUncached): a peer
  // GPU writes them over xGMI while a kernel here spins on them, and plain
  // (coarse-grained) hipMalloc memory is only coherent at dispatch
  // boundaries -- a line held in this device's L2 could hide the write.
  void create(size_t n) {
    nflags = std::max<size_t>(n, 1);
    hip_check(hipExtMallocWithFlags((void **)&local, nflags * sizeof(uint32_t), hipDeviceMallocUncached),
              "hipExtMallocWithFlags(flags, uncached)");
    hip_check(hipMemset(local, 0, nflags * sizeof(uint32_t)), "hipMemset(flags)");
    hip_check(hipHostMalloc((void **)&err, sizeof(uint32_t), hipHostMallocCoherent), "hipHostMalloc(err)");
    *err = 0;
    hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize(flags)");
    IpcExport mine = ipc_export(local, -1);
    std::vector<IpcExport> all(numproc);
    mpi_check(MPI_Allgather(&mine, sizeof(IpcExport), MPI_BYTE, all.data(), sizeof(IpcExport), MPI_BYTE, comm_mpi),
              "MPI_Allgather(flags)");
    peer.assign(numproc, nullptr);
    for (int r = 0; r < numproc; r++) peer[r] = r == myid ? local : (uint32_t *)ipc_import(r, all[r], held);
  }
  // Close the mappings of the peers' arrays (before the peers free them).
  void close() { ipc_release(held); }
  ~FlagSpace() {
    ipc_release(held);
    if (err) (void)hipHostFree(err);
    if (local) (void)hipFree(local);
  }
};

// Seconds a stream-ordered wait may spin before it reports a timeout
// (HICCL_SIGNAL_TIMEOUT, default 60).
inline double signal_timeout() {
  static double t = [] {
    const char *e = std::getenv("HICCL_SIGNAL_TIMEOUT");
    double v = e ? std::atof(e) : 60.0;
    return v > 0 ? v : 60.0;
  }();
  return t;
}

// Stream-ordered signalling is queued: consecutive signal/wait steps with
// nothing else between them on the stream (a step's done tokens and the next
// step's readies) go out as ONE launch of ordered phases
// (hiccl_signal_wait_phases) -- the same order of every operation on the
// stream with fewer kernel boundaries.  flush_signals() must run before
// anything else is enqueued on that stream and before it is synchronised or
// its capture ends; every such point of the transport and of HiCCL::Comm
// calls it.
struct PendingSignals {
  struct Phase {
    std::vector<uint32_t *> sig, wait;
    uint32_t epoch;
    std::function<uint32_t()> epoch_now;  // the owner's epoch for this phase at any later launch (step programs)
  };
  std::vector<Phase> phases;
  const uint32_t *epoch_dev = nullptr;
  uint32_t *err = nullptr;
  hipStream_t stream = nullptr;
};

// Per host thread: a pipeline is enqueued (and flushed) by one thread, and
// pipelines of different threads never share a queue.
inline PendingSignals &pending_signals() {
  static thread_local PendingSignals p;
  return p;
}

// Programs (HiCCL::Comm, stream-ordered mode; hiccl_program_*): while a
// recorder is set on this thread, flush_signals() and the transport's and
// computes' plan launches APPEND to the recorder instead of enqueueing.  The
// recorder folds every group of queued phases into the program of the unit
// batch that follows it (one launch: phases, then units), so a pipeline
// becomes a list of programs with no separate signal/wait launches.  A
// phase's epoch is not fixed in the program: epoch_of[p]() gives it at each
// launch (the owning transport's current epoch).
struct StepRecorder {
  struct Launch {
    hiccl_program_t *prog;
    std::vector<std::function<uint32_t()>> epoch_of;
  };
  std::vector<Launch> launches;  // finished programs, in stream order
  int dtype = 0, device = 0, max_wg = 0;
  hiccl_program_t *cur = nullptr;
  std::vector<std::function<uint32_t()>> cur_epochs;
  bool cur_units = false;
  int last = 0;                      // kind of the last batch appended: 1 copies, 2 computes
  const void *last_owner = nullptr;  // the transport whose copies were appended last
  bool join_all_copies = false;      // one batch for the copies of every transport of a step

  void open() {
    if (cur) return;
    if (hiccl_program_create(&cur, dtype, device)) die("program", hiccl_last_error());
    if (max_wg && hiccl_program_set_max_workgroups(cur, max_wg)) die("program", hiccl_last_error());
  }
  // A step's computes are complete: the next step's computes start a new
  // batch even when nothing of this rank is recorded between them (a step
  // with computes but no phase or copy of its own) -- the reference waits
  // for each step's computes before the next step starts (comm.h:203-204).
  void end_step() { last = 0; }
  void close() {
    if (!cur) return;
    launches.push_back(Launch{cur, std::move(cur_epochs)});
    cur = nullptr;
    cur_epochs.clear();
    cur_units = false;
    last = 0;
  }
};
inline StepRecorder *&step_recorder() {
  static thread_local StepRecorder *r = nullptr;
  return r;
}

// Append plan `p` to the recording: copies of one transport's execution
// (move + self plans) share a batch, so do the computes of a step (the
// reference starts them together on separate streams, comm.h:198-202, so
// they are independent); anything else starts a new program, i.e. runs
// after the previous batch has completed (a kernel boundary).
inline void record_plan(hiccl_reduce_plan_t *p, int kind, const void *owner) {
  StepRecorder *r = step_recorder();
  const bool join = r->cur_units && r->last == kind && (kind == 2 || r->last_owner == owner);
  if (r->cur_units && !join) r->close();
  r->open();
  if (hiccl_program_add_plan(r->cur, p)) die("program", hiccl_last_error());
  r->cur_units = true;
  r->last = kind;
  r->last_owner = owner;
}

inline void flush_signals() {
  PendingSignals &p = pending_signals();
  if (p.phases.empty()) return;
  if (StepRecorder *r = step_recorder()) {
    if (r->cur_units) r->close();  // these phases guard the NEXT batch
    for (auto &ph : p.phases) {
      r->open();
      if (hiccl_program_num_phases(r->cur) >= 64) {  // a program holds 64 phases: the rest go first in the next
        r->close();
        r->open();
      }
      if (hiccl_program_add_signal(r->cur, ph.sig.data(), (int)ph.sig.size(),
                                   (const uint32_t *const *)ph.wait.data(), (int)ph.wait.size()))
        die("program", hiccl_last_error());
      r->cur_epochs.push_back(ph.epoch_now);
    }
    p.phases.clear();
    return;
  }
  std::vector<hiccl_signal_phase_t> ph(p.phases.size());
  for (size_t i = 0; i < ph.size(); i++) {
    ph[i].sig = p.phases[i].sig.data();
    ph[i].nsig = (int)p.phases[i].sig.size();
    ph[i].wait = (const uint32_t *const *)p.phases[i].wait.data();
    ph[i].nwait = (int)p.phases[i].wait.size();
    ph[i].epoch = p.phases[i].epoch;
  }
  int e = hiccl_signal_wait_phases(ph.data(), (int)ph.size(), p.epoch_dev, p.err, signal_timeout(), p.stream);
  p.phases.clear();
  if (e) die("hiccl_signal_wait", hiccl_last_error());
}

// epoch_dev != NULL (graph capture): the epoch used is epoch + *epoch_dev at run time.
inline void signal_wait(const std::vector<uint32_t *> &sig, const std::vector<uint32_t *> &wait, uint32_t epoch,
                        const uint32_t *epoch_dev, uint32_t *err, hipStream_t stream,
                        std::function<uint32_t()> epoch_now = nullptr) {
  if (sig.empty() && wait.empty()) return;
  PendingSignals &p = pending_signals();
  if (!p.phases.empty() && (p.epoch_dev != epoch_dev || p.err != err || p.stream != stream)) flush_signals();
  p.epoch_dev = epoch_dev;
  p.err = err;
  p.stream = stream;
  p.phases.push_back(PendingSignals::Phase{sig, wait, epoch, std::move(epoch_now)});
}
#endif


// ------------------------------------------------------ point-to-point ----
//
// Comm<T>: a persistent set of registered transfers on one library,
// SPMD-registered (every rank calls add for every transfer, in the same
// order; only the two endpoints act), started and completed as a unit.
// Call sites in the reference: command.h:122,132 (construction, add),
// comm.h:190,197 (start, wait), command.h:17-37 (measure, numsend/numrecv).
//
// Roles per transfer: the MOVER issues the copy (the sender for IPC "put",
// the receiver for IPC_get), the OWNER is the other endpoint (it owns the
// destination of a put / the source of a get).  Host-driven mode: the owner
// posts a zero-byte "ready" to the mover at start(), the mover copies after
// it and posts "done", the owner waits for "done" in wait().  Stream-ordered
// mode: the same two signals are device flags (ready in the mover's
// FlagSpace slot 2*(base+j), done in the owner's slot 2*(base+j)+1), set and
// awaited by hiccl_signal_wait on the rank's stream around the copies.
constexpr int kDoneTag = 16000;

template <typename T>
class Comm {
 public:
  library lib;
  int numsend = 0;
  int numrecv = 0;

  explicit Comm(library lib) : lib(lib) {
#ifdef HICCL_PORT_HOST
    if (this->lib != dummy) this->lib = MPI;
#else
    streamed = stream_ordered;
    if (this->lib == XCCL && !xccl_on()) this->lib = IPC;  // no RCCL (see xccl_setup): the xGMI IPC path
    if (streamed && this->lib == MPI) this->lib = IPC;  // one node: move device bytes directly
    stream = transport_stream();
#endif
  }

  ~Comm() {
#ifndef HICCL_PORT_HOST
    if (!held.empty()) (void)hipStreamSynchronize(stream);  // no copy still reads or writes a mapping
    for (auto &x : xfers)
      if (x.staging) (void)hipHostFree(x.staging);
    if (moveplan) hiccl_reduce_plan_destroy(moveplan);
    if (selfplan) hiccl_reduce_plan_destroy(selfplan);
    ipc_release(held);
#endif
  }

  Comm(const Comm &) = delete;
  Comm &operator=(const Comm &) = delete;

  // Register one transfer: count elements from sendbuf+sendoffset on rank
  // sendid to recvbuf+recvoffset on rank recvid.  Pointers need only be
  // valid on their owning rank.
  //
  // `fused` (IPC / IPC_get only, decided identically on every rank): the
  // bytes are not moved at all.  The receiver maps the sender's buffer and
  // its compute reads it in place (fused_source); the sender's ready token
  // precedes the compute and the receiver's done token follows it (finish /
  // enqueue_tail), so the sender keeps the buffer intact until then.
  void add(T *sendbuf, size_t sendoffset, T *recvbuf, size_t recvoffset, size_t count, int sendid,
           int recvid, bool fused = false) {
    Xfer x;
    x.src = sendbuf ? sendbuf + sendoffset : nullptr;
    x.dst = recvbuf ? recvbuf + recvoffset : nullptr;
    x.count = count;
    x.sendid = sendid;
    x.recvid = recvid;
    // tags stay below MPI's guaranteed MPI_TAG_UB (32767): the done token of
    // a transfer uses tag + kDoneTag
    x.tag = (int)(xfers.size() % kDoneTag);
    if (myid == sendid) numsend++;
    if (myid == recvid) numrecv++;
    if (lib == dummy || count == 0 || lib == XCCL) {  // XCCL: RCCL needs no registration
      xfers.push_back(x);
      return;
    }
#ifndef HICCL_PORT_HOST
    x.fused = fused && sendid != recvid && (lib == IPC || lib == IPC_get);
    if (sendid != recvid && (lib == IPC || lib == IPC_get)) {
      // the mover needs a mapping of the owner's buffer
      const int owner = owner_of(x), mover = mover_of(x);
      if (myid == owner) {
        T *mine = owner == x.sendid ? x.src : x.dst;
        IpcExport e = ipc_export(mine, mover);
        const uint64_t saved = e.recycled ? ipc_probe_begin(e, mine, count * sizeof(T)) : 0;
        mpi_check(MPI_Send(&e, sizeof(e), MPI_BYTE, mover, x.tag, comm_mpi), "MPI_Send(ipc)");
        if (e.probe) {
          int ok = 0;
          mpi_check(MPI_Recv(&ok, 1, MPI_INT, mover, x.tag, comm_mpi, MPI_STATUS_IGNORE), "MPI_Recv(probe)");
          ipc_probe_finish(e, mine, saved);
          if (!ok)
            die("transport", "rank " + std::to_string(mover) + "'s IPC mapping of a reallocated buffer of this rank "
                "does not reach it (the peer closed an earlier mapping of this freed and reused address: raise "
                "HICCL_IPC_RETIRED_MAX, or keep the buffers allocated across communicators)");
        }
      }
      if (myid == mover) {
        IpcExport e;
        std::memset(&e, 0, sizeof(e));
        MPI_Status st;
        mpi_check(MPI_Recv(&e, sizeof(e), MPI_BYTE, owner, x.tag, comm_mpi, &st), "MPI_Recv(ipc)");
        int got = 0;
        MPI_Get_count(&st, MPI_BYTE, &got);
        if (got != (int)sizeof(e)) die("transport", "IPC handle exchange matched a message of " + std::to_string(got) + " bytes");
        x.remote = ipc_import(owner, e, held);
        if (e.probe) {
          std::string seen;
          const size_t have = ipc_opened().at(IpcKey{owner, (uintptr_t)e.base}).bytes;  // 0: unknown
          int bad = ipc_probe_check(e, x.remote, !have ? SIZE_MAX : have > e.offset ? have - (size_t)e.offset : 0, &seen);
          int ok = bad == 0;
          if (ipc_debug()) ipc_note("[ipc %d] probe peer %d base %#llx: %d\n", myid, owner,
                                    (unsigned long long)e.base, bad);
          mpi_check(MPI_Send(&ok, 1, MPI_INT, owner, x.tag, comm_mpi), "MPI_Send(probe)");
          if (!ok) die("transport", "this rank's IPC mapping of a reallocated buffer of rank " + std::to_string(owner) +
                                    " does not reach it (" + seen + ")");
        }
      }
    }
    if (sendid != recvid && lib == MPI && (myid == sendid || myid == recvid))
      hip_check(hipHostMalloc((void **)&x.staging, count * sizeof(T), hipHostMallocDefault), "hipHostMalloc");
#endif
    xfers.push_back(x);
  }

  // On the receiver of a fused transfer whose destination is `dst`: the
  // mapping of the sender's buffer, which the compute reads instead.
  T *fused_source(const T *dst) const {
    for (auto &x : xfers)
      if (x.fused && x.recvid == myid && x.dst == dst) return reinterpret_cast<T *>(x.remote);
    return nullptr;
  }

#ifndef HICCL_PORT_HOST
  // Stream-ordered mode: assign flag slots [2*base, 2*(base+size())) of fs.
  void bind(FlagSpace *fs, size_t base) {
    flags = fs;
    pre_sig.clear();
    pre_wait.clear();
    post_sig.clear();
    post_wait.clear();
    tail_sig.clear();
    tail_wait.clear();
    for (size_t j = 0; j < xfers.size(); j++) {
      const Xfer &x = xfers[j];
      // XCCL: RCCL orders its sends and receives on the stream itself
      if (lib == dummy || lib == XCCL || x.count == 0 || x.sendid == x.recvid) continue;
      const int owner = owner_of(x), mover = mover_of(x);
      const size_t ready = 2 * (base + j), done = ready + 1;
      if (myid == owner) {
        pre_sig.push_back(fs->peer[mover] + ready);
        (x.fused ? tail_wait : post_wait).push_back(fs->local + done);
      }
      if (myid == mover) {
        pre_wait.push_back(fs->local + ready);
        (x.fused ? tail_sig : post_sig).push_back(fs->peer[owner] + done);
      }
    }
  }

  // Enqueue one execution on `s` without waiting: owners signal ready,
  // movers wait for ready, copy, signal done, owners wait for done.  The
  // done tokens of fused transfers follow the step's compute: enqueue_tail.
  void enqueue(hipStream_t s) {
    ++epoch;
    if (lib == XCCL) {
      xccl_group(s);
      return;
    }
    signal_wait(pre_sig, pre_wait, sig_epoch(), graph_epoch, flags->err, s, epoch_fn());
    launch_copies(s);
    signal_wait(post_sig, post_wait, sig_epoch(), graph_epoch, flags->err, s, epoch_fn());
  }
  void enqueue_tail(hipStream_t s) {
    signal_wait(tail_sig, tail_wait, sig_epoch(), graph_epoch, flags->err, s, epoch_fn());
  }
  // enqueue() in three parts, so that a step's transports can be issued the
  // way the reference starts them -- all together (comm.h:188-191) -- every
  // ready phase first, then every copy, then every done phase (programs).
  void enqueue_pre(hipStream_t s) {
    ++epoch;
    signal_wait(pre_sig, pre_wait, sig_epoch(), graph_epoch, flags->err, s, epoch_fn());
  }
  void enqueue_copies(hipStream_t s) { launch_copies(s); }
  void enqueue_post(hipStream_t s) {
    signal_wait(post_sig, post_wait, sig_epoch(), graph_epoch, flags->err, s, epoch_fn());
  }
  // A recorded step program runs instead of enqueue(): the execution still
  // counts (the program's phases read sig_epoch() at each launch).
  void advance() { ++epoch; }
  // Can this transport's executions be recorded into a step program?
  bool recordable() const { return lib != XCCL; }

  // hipGraph capture of stream-ordered executions (HiCCL::Comm::run with
  // HICCL_GRAPH=1): while `ctr` is set, every wait is enqueued as
  // (epoch before this execution) + *ctr, where *ctr is the replay number
  // (1, 2, ...) bumped by the graph's first node; the host epoch then
  // advances by one per replay (end_capture undoes the capture's own ++).
  void begin_capture(const uint32_t *ctr) { graph_epoch = ctr; }
  void end_capture() {
    graph_epoch = nullptr;
    --epoch;
  }
  void replayed() { ++epoch; }
  uint32_t epoch_now() const { return epoch; }

  bool stream_mode() const { return streamed; }
#endif

  void start() {
#ifndef HICCL_PORT_HOST
    setup_gpu();
    if (streamed) {
      if (!flags) die("transport", "stream-ordered Comm used before bind()");
      enqueue(stream);
      enqueue_tail(stream);  // standalone use (measure): no compute in between
      flush_signals();
      return;
    }
    if (lib == XCCL) {
      xccl_group(stream);
      return;
    }
    build_plans();
#endif
    reqs.clear();
    movers.clear();
    readers.clear();
    tail_reqs.clear();
    issued = false;
#ifndef HICCL_PORT_HOST
    if (selfplan) {
      launch_plan(selfplan, stream, "self copies");
      issued = true;
    }
#endif
    for (auto &x : xfers) {
      if (lib == dummy || x.count == 0) continue;
      const bool me_send = myid == x.sendid, me_recv = myid == x.recvid;
      if (!me_send && !me_recv) continue;
      if (x.sendid == x.recvid) {  // self transfer (device: in the batched self-copy below)
#ifdef HICCL_PORT_HOST
        std::memmove(x.dst, x.src, x.count * sizeof(T));
#endif
        continue;
      }
      const int peer = me_send ? x.recvid : x.sendid;
      if (lib == MPI) {
#ifdef HICCL_PORT_HOST
        post(me_send ? MPI_Isend(x.src, bytes(x), MPI_BYTE, peer, x.tag, comm_mpi, next())
                     : MPI_Irecv(x.dst, bytes(x), MPI_BYTE, peer, x.tag, comm_mpi, next()));
#else
        if (me_send) {
          hip_check(hipMemcpyAsync(x.staging, x.src, bytes(x), hipMemcpyDeviceToHost, stream), "stage D2H");
          hip_check(hipStreamSynchronize(stream), "stage sync");
          post(MPI_Isend(x.staging, bytes(x), MPI_BYTE, peer, x.tag, comm_mpi, next()));
        } else {
          post(MPI_Irecv(x.staging, bytes(x), MPI_BYTE, peer, x.tag, comm_mpi, next()));
        }
#endif
        continue;
      }
#ifndef HICCL_PORT_HOST
      const bool mover = myid == mover_of(x);
      if (mover) {
        (x.fused ? readers : movers).push_back({&x, (int)reqs.size()});
        post(MPI_Irecv(nullptr, 0, MPI_BYTE, peer, x.tag, comm_mpi, next()));  // ready
      } else {
        post(MPI_Isend(nullptr, 0, MPI_BYTE, peer, x.tag, comm_mpi, next()));  // ready
        if (x.fused) {
          tail_reqs.emplace_back();  // done: after the reader's compute, in finish()
          post(MPI_Irecv(nullptr, 0, MPI_BYTE, peer, x.tag + kDoneTag, comm_mpi, &tail_reqs.back()));
        } else {
          post(MPI_Irecv(nullptr, 0, MPI_BYTE, peer, x.tag + kDoneTag, comm_mpi, next()));  // done
        }
      }
#endif
    }
  }

  void wait() {
#ifndef HICCL_PORT_HOST
    setup_gpu();
    if (streamed || lib == XCCL) {
      flush_signals();
      hip_check(hipStreamSynchronize(stream), "transport stream sync");
      if (flags && *flags->err) die("transport", "stream-ordered signal timed out (peer never signalled)");
      return;
    }
    for (auto &m : movers) mpi_check(MPI_Wait(&reqs[m.req], MPI_STATUS_IGNORE), "MPI_Wait(ready)");
    for (auto &m : readers) mpi_check(MPI_Wait(&reqs[m.req], MPI_STATUS_IGNORE), "MPI_Wait(ready)");
    if (!movers.empty() && moveplan) launch_plan(moveplan, stream, "IPC moves");  // every move, one kernel
    if (issued || !movers.empty()) hip_check(hipStreamSynchronize(stream), "transport stream sync");
    for (auto &m : movers) {
      const Xfer &x = *m.x;
      const int peer = myid == x.sendid ? x.recvid : x.sendid;
      post(MPI_Isend(nullptr, 0, MPI_BYTE, peer, x.tag + kDoneTag, comm_mpi, next()));  // done
    }
#endif
    if (!reqs.empty()) mpi_check(MPI_Waitall((int)reqs.size(), reqs.data(), MPI_STATUSES_IGNORE), "MPI_Waitall");
    reqs.clear();
#ifndef HICCL_PORT_HOST
    if (lib == MPI) {  // unstage received bytes
      for (auto &x : xfers)
        if (myid == x.recvid && x.sendid != x.recvid && x.count)
          hip_check(hipMemcpyAsync(x.dst, x.staging, bytes(x), hipMemcpyHostToDevice, stream), "unstage H2D");
      hip_check(hipStreamSynchronize(stream), "unstage sync");
    }
#endif
  }

  // After the step's compute (host-driven mode): readers of fused transfers
  // release the senders' buffers; senders wait for that release.
  void finish() {
#ifndef HICCL_PORT_HOST
    if (streamed) return;
    for (auto &m : readers) {
      const int peer = m.x->sendid;
      tail_reqs.emplace_back();
      post(MPI_Isend(nullptr, 0, MPI_BYTE, peer, m.x->tag + kDoneTag, comm_mpi, &tail_reqs.back()));
    }
    if (!tail_reqs.empty())
      mpi_check(MPI_Waitall((int)tail_reqs.size(), tail_reqs.data(), MPI_STATUSES_IGNORE), "MPI_Waitall(done)");
    tail_reqs.clear();
    readers.clear();
#endif
  }

  // Per-step transport micro-benchmark (CommBench::Comm::measure call site:
  // command.h:21).  Prints min/median/max like the reference's tables.
  void measure(int warmup, int numiter, size_t count) {
    std::vector<double> t;
    for (int it = -warmup; it < numiter; it++) {
      MPI_Barrier(comm_mpi);
      double t0 = MPI_Wtime();
      start();
      wait();
      finish();
      double dt = MPI_Wtime() - t0;
      MPI_Allreduce(MPI_IN_PLACE, &dt, 1, MPI_DOUBLE, MPI_MAX, comm_mpi);
      if (it >= 0) t.push_back(dt);
    }
    std::sort(t.begin(), t.end());
    if (myid == printid && !t.empty()) {
      const double data = (double)count * sizeof(T);
      std::printf("%s transfers: min %.4e s, median %.4e s, max %.4e s, %.3f GB/s (median)\n", lib_name(lib),
                  t.front(), t[t.size() / 2], t.back(), data / t[t.size() / 2] / 1e9);
    }
  }

  size_t size() const { return xfers.size(); }

 private:
  struct Xfer {
    T *src = nullptr;
    T *dst = nullptr;
    char *remote = nullptr;  // mapping of the owner's buffer (IPC: its dst; IPC_get: its src)
    T *staging = nullptr;    // pinned host staging (MPI with device memory)
    size_t count = 0;
    int sendid = 0, recvid = 0, tag = 0;
    bool fused = false;  // no bytes move: the receiver's compute reads `remote`
  };
  // IPC: the sender moves into the receiver's buffer; IPC_get and fused
  // transfers: the receiver maps the sender's buffer.
  int owner_of(const Xfer &x) const { return lib == IPC && !x.fused ? x.recvid : x.sendid; }
  int mover_of(const Xfer &x) const { return lib == IPC && !x.fused ? x.sendid : x.recvid; }
  struct Mover {
    Xfer *x;
    int req;
  };
  std::vector<Xfer> xfers;
  std::vector<MPI_Request> reqs;
  std::vector<Mover> movers, readers;
  std::vector<MPI_Request> tail_reqs;
  bool issued = false;  // async device work enqueued by start()
#ifndef HICCL_PORT_HOST
  hipStream_t stream = nullptr;
  bool streamed = false;
  FlagSpace *flags = nullptr;
  std::vector<IpcKey> held;  // the owners' buffers this rank maps (ipc_import)
  uint32_t epoch = 0;
  const uint32_t *graph_epoch = nullptr;  // set while a graph is being captured
  uint32_t sig_epoch() const { return graph_epoch ? epoch - 1 : epoch; }
  std::function<uint32_t()> epoch_fn() const {
    return [this] { return sig_epoch(); };
  }
  std::vector<uint32_t *> pre_sig, pre_wait, post_sig, post_wait, tail_sig, tail_wait;
  // batched exact copies (HICCL_BYTES plans): the bytes this rank moves to or
  // from peers, and its self transfers -- one kernel each per execution
  hiccl_reduce_plan_t *moveplan = nullptr, *selfplan = nullptr;
  bool planned = false;

  void build_plans() {
    if (planned) return;
    planned = true;
    if (lib == dummy) return;
    for (const Xfer &x : xfers) {
      if (!x.count) continue;
      if (lib == XCCL && xccl_self_on_rccl()) continue;  // every transfer of the level is RCCL's (xccl_group)
      const bool self = x.sendid == x.recvid && x.sendid == myid;
      const bool move = x.sendid != x.recvid && !x.fused && (lib == IPC || lib == IPC_get) && myid == mover_of(x);
      if (!self && !move) continue;
      hiccl_reduce_plan_t *&p = self ? selfplan : moveplan;
      if (!p) {
        if (hiccl_reduce_plan_create(&p, HICCL_BYTES, mydevice)) die("transport", hiccl_last_error());
        // a put writes the peer's buffer, a get reads it: system-scope
        // stores / loads, so the bytes are in the peer's HBM when the done
        // token says so and no stale line of it is read back
        // (hiccl_reduce_plan_set_peer)
        if (!self && hiccl_reduce_plan_set_peer(p, lib == IPC ? HICCL_PEER_STORES : HICCL_PEER_LOADS))
          die("transport", hiccl_last_error());
      }
      const void *src = self || lib == IPC ? (const void *)x.src : (const void *)x.remote;
      void *dst = self || lib == IPC_get ? (void *)x.dst : (void *)x.remote;
      if (lib == IPC && !self) dst = x.remote;
      if (ipc_debug())
        ipc_note("[ipc %d] %s copy %p -> %p, %zu B (transfer %d -> %d)\n", myid, self ? "self" : "move", src, dst,
                 x.count * sizeof(T), x.sendid, x.recvid);
      if (hiccl_reduce_plan_add(p, dst, &src, 1, x.count * sizeof(T))) die("transport copy plan", hiccl_last_error());
    }
  }

  // the transport synchronises its stream (or orders it by flags), never a
  // plan's completion event: enqueue without one
  void launch_plan(hiccl_reduce_plan_t *p, hipStream_t s, const char *what) {
    flush_signals();  // queued signal/wait steps precede this kernel on the stream
    if (StepRecorder *r = step_recorder()) return record_plan(p, 1, r->join_all_copies ? nullptr : this);
    if (hiccl_reduce_plan_enqueue(p, s)) die(what, hiccl_last_error());
  }

  void launch_copies(hipStream_t s) {
    build_plans();
    if (moveplan) launch_plan(moveplan, s, "IPC moves");
    if (selfplan) launch_plan(selfplan, s, "self copies");
  }

  // XCCL level: this rank's self copies (one batched kernel) and its sends
  // and receives as one RCCL group on `s`, in registration order (every
  // rank registers the same transfers in the same order, so each pair's
  // sends and receives match).
  void xccl_group(hipStream_t s) {
    flush_signals();
    build_plans();
    if (selfplan) launch_plan(selfplan, s, "self copies");
#ifdef HICCL_WITH_RCCL
    const bool self_too = xccl_self_on_rccl();
    auto on_rccl = [&](const Xfer &x) {
      return x.count && (x.sendid != x.recvid || self_too) && (myid == x.sendid || myid == x.recvid);
    };
    bool any = false;
    for (const Xfer &x : xfers) any = any || on_rccl(x);
    if (!any) return;
    nccl_check(ncclGroupStart(), "ncclGroupStart");
    for (const Xfer &x : xfers) {
      if (!on_rccl(x)) continue;
      if (myid == x.sendid)
        nccl_check(ncclSend(x.src, x.count * sizeof(T), ncclUint8, x.recvid, xccl_comm(), s), "ncclSend");
      if (myid == x.recvid)
        nccl_check(ncclRecv(x.dst, x.count * sizeof(T), ncclUint8, x.sendid, xccl_comm(), s), "ncclRecv");
    }
    nccl_check(ncclGroupEnd(), "ncclGroupEnd");
#endif
  }
#endif

  static int bytes(const Xfer &x) {
    const size_t b = x.count * sizeof(T);
    if (b > (size_t)2147483647) die("transport", "message above 2 GiB: raise pipedepth");
    return (int)b;
  }
  MPI_Request *next() {
    reqs.emplace_back();
    return &reqs.back();
  }
  static void post(int e) { mpi_check(e, "MPI post"); }
};

}  // namespace CommBench

#endif  // HICCL_TRANSPORT_H
