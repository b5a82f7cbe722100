// loopback_rccl.cpp — a stand-in for the six RCCL entry points the engine resolves at run time (RcclApi in
// csrc/ahmc_multi_host.hpp), so that R processes sharing ONE GPU can run everything the engine does around its collectives.
// Test infrastructure only: nothing under advancedhmc.jl_amd/ links or names it; a worker process selects it with AHMC_RCCL_LIB.
//
// Exchange: the ranks meet in a file the parent test created (zero-filled, path in LOOPBACK_RCCL_FILE), mapped MAP_SHARED by
// every rank.  The file is cut into regions of REGION_BYTES after a page of global header; the first four bytes of a
// ncclUniqueId name the region a communicator lives in (the rest of the 128 bytes is opaque here as it is to the engine), so
// communicators made from different ids never share state.  A region = one page of control words + MAX_RANKS slots.
//
// A collective: hipStreamSynchronize(stream); device → host copy of the send buffer into the rank's slot; barrier; every rank
// reduces / concatenates the slots IN RANK ORDER on the host (so every rank gets the same bits); host → device copy into the
// receive buffer; second barrier (no slot is overwritten before every rank has read it).  In-place calls work: the send buffer
// was copied out before anything is written.
//
// Every wait has a deadline (LOOPBACK_RCCL_DEADLINE_S, default 60 s): a rank that waits longer returns ncclSystemError and the
// communicator stays broken.  Waiters sleep on host memory; nothing is launched on the GPU while they wait.
//
// -DLOOPBACK_HOST_BUFFERS: the two copies are memcpy and no HIP call is made (the buffers are host memory): the exchange logic
// on a machine without a GPU (tests/host_ref/loopback_rccl_driver.cpp).
#include <rccl/rccl.h>

#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <time.h>
#include <unistd.h>

#include <atomic>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <new>

namespace {

constexpr size_t GLOBAL_BYTES = 4096;          // global header: the counter ncclGetUniqueId hands regions out from
constexpr size_t REGION_BYTES = size_t(2) << 20;
constexpr size_t CONTROL_BYTES = 4096;
constexpr int MAX_RANKS = 8;
constexpr size_t SLOT_BYTES = (REGION_BYTES - CONTROL_BYTES) / MAX_RANKS;   // 261632 B: 32704 doubles per rank

struct Meta {           // what a rank announces before the first barrier of a collective
  uint64_t seq;         // collectives this communicator has served before this one
  uint32_t kind;        // 1 all-reduce, 2 all-gather
  uint32_t dtype, op;
  uint32_t valid;       // the rank itself found the call supported and its payload inside a slot
  uint64_t count;
};

struct Control {
  std::atomic<uint32_t> arrived;
  std::atomic<uint32_t> sense;
  uint32_t pad[14];
  Meta meta[MAX_RANKS];
};
static_assert(sizeof(Control) <= CONTROL_BYTES, "control page");
static_assert(std::atomic<uint32_t>::is_always_lock_free, "the barrier words live in shared memory");

struct Global {
  std::atomic<uint32_t> ids_made;
};

struct Mapping {
  char* base = nullptr;
  size_t bytes = 0;
  size_t regions = 0;
};

struct Comm {
  uint32_t magic;
  int n, rank;
  uint32_t sense;       // local sense of the sense-reversing barrier
  uint64_t seq;
  bool broken;
  Control* ctl;
  char* slots;
};
constexpr uint32_t MAGIC = 0x4c42434bu;

std::atomic<int> g_live{0};
std::atomic<long> g_calls[3];

Mapping& mapping() {
  static Mapping m = [] {
    Mapping x;
    const char* path = getenv("LOOPBACK_RCCL_FILE");
    if (!path) return x;
    const int fd = open(path, O_RDWR);
    if (fd < 0) return x;
    struct stat st;
    if (fstat(fd, &st) == 0 && (size_t)st.st_size >= GLOBAL_BYTES + REGION_BYTES) {
      void* p = mmap(nullptr, (size_t)st.st_size, PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0);
      if (p != MAP_FAILED) {
        x.base = static_cast<char*>(p);
        x.bytes = (size_t)st.st_size;
        x.regions = (x.bytes - GLOBAL_BYTES) / REGION_BYTES;
      }
    }
    close(fd);
    return x;
  }();
  return m;
}

double deadline_seconds() {
  const char* e = getenv("LOOPBACK_RCCL_DEADLINE_S");
  const double v = e ? atof(e) : 0.0;
  return v > 0 ? v : 60.0;
}

double now() {
  timespec t;
  clock_gettime(CLOCK_MONOTONIC, &t);
  return (double)t.tv_sec + 1e-9 * (double)t.tv_nsec;
}

// sense-reversing barrier over the communicator's n ranks; false when the deadline passed (the communicator is then broken:
// its count no longer means anything)
bool barrier(Comm* c) {
  c->sense ^= 1u;
  const uint32_t mine = c->sense;
  if (c->ctl->arrived.fetch_add(1, std::memory_order_acq_rel) + 1 == (uint32_t)c->n) {
    c->ctl->arrived.store(0, std::memory_order_relaxed);
    c->ctl->sense.store(mine, std::memory_order_release);
    return true;
  }
  const double end = now() + deadline_seconds();
  timespec nap{0, 50 * 1000};
  while (c->ctl->sense.load(std::memory_order_acquire) != mine) {
    if (now() > end) { c->broken = true; return false; }
    nanosleep(&nap, nullptr);
  }
  return true;
}

size_t elem_bytes(ncclDataType_t t) { return t == ncclDouble ? 8 : t == ncclFloat ? 4 : 0; }

ncclResult_t to_host(void* dst, const void* src, size_t bytes, hipStream_t stream) {
#ifdef LOOPBACK_HOST_BUFFERS
  (void)stream;
  memcpy(dst, src, bytes);
#else
  if (hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, stream) != hipSuccess) return ncclUnhandledCudaError;
  if (hipStreamSynchronize(stream) != hipSuccess) return ncclUnhandledCudaError;
#endif
  return ncclSuccess;
}

ncclResult_t to_device(void* dst, const void* src, size_t bytes, hipStream_t stream) {
#ifdef LOOPBACK_HOST_BUFFERS
  (void)stream;
  memcpy(dst, src, bytes);
#else
  if (hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, stream) != hipSuccess) return ncclUnhandledCudaError;
  if (hipStreamSynchronize(stream) != hipSuccess) return ncclUnhandledCudaError;
#endif
  return ncclSuccess;
}

template <class F>
void reduce_slots(const Comm* c, size_t count, double* out, F f) {
  const double* s0 = reinterpret_cast<const double*>(c->slots);
  for (size_t i = 0; i < count; ++i) out[i] = s0[i];
  for (int r = 1; r < c->n; ++r) {   // rank order: the same sequence of operations on every rank
    const double* s = reinterpret_cast<const double*>(c->slots + (size_t)r * SLOT_BYTES);
    for (size_t i = 0; i < count; ++i) out[i] = f(out[i], s[i]);
  }
}

ncclResult_t collective(uint32_t kind, const void* send, void* recv, size_t count, ncclDataType_t dtype, ncclRedOp_t op, ncclComm_t comm_,
                        hipStream_t stream) {
  Comm* c = reinterpret_cast<Comm*>(comm_);
  if (!c || c->magic != MAGIC) return ncclInvalidArgument;
  if (c->broken) return ncclSystemError;
  const size_t eb = elem_bytes(dtype);
  bool valid = send && recv && eb != 0;
  if (kind == 1) valid = valid && dtype == ncclDouble && (op == ncclSum || op == ncclMax);
  const size_t bytes = count * eb;
  valid = valid && count <= SLOT_BYTES / 8 && bytes <= SLOT_BYTES;
#ifndef LOOPBACK_HOST_BUFFERS
  if (hipStreamSynchronize(stream) != hipSuccess) return ncclUnhandledCudaError;
#endif
  ncclResult_t rc = ncclSuccess;
  if (valid && bytes) rc = to_host(c->slots + (size_t)c->rank * SLOT_BYTES, send, bytes, stream);
  Meta& m = c->ctl->meta[c->rank];
  m.seq = c->seq;
  m.kind = kind;
  m.dtype = (uint32_t)dtype;
  m.op = kind == 1 ? (uint32_t)op : 0u;
  m.valid = (valid && rc == ncclSuccess) ? 1u : 0u;
  m.count = (uint64_t)count;
  if (!barrier(c)) return ncclSystemError;
  // every rank reads the same n announcements, so every rank comes to the same verdict
  bool agree = true;
  for (int r = 0; r < c->n; ++r) {
    const Meta& o = c->ctl->meta[r];
    agree = agree && o.valid == 1u && o.seq == m.seq && o.kind == m.kind && o.dtype == m.dtype && o.op == m.op && o.count == m.count;
  }
  if (agree && bytes) {
    if (kind == 1) {
      double* tmp = new (std::nothrow) double[count];
      if (!tmp) {
        rc = ncclSystemError;
      } else {
        if (op == ncclSum) reduce_slots(c, count, tmp, [](double a, double b) { return a + b; });
        else reduce_slots(c, count, tmp, [](double a, double b) { return a > b ? a : b; });
        rc = to_device(recv, tmp, bytes, stream);
        delete[] tmp;
      }
    } else {
      for (int r = 0; r < c->n && rc == ncclSuccess; ++r)
        rc = to_device(static_cast<char*>(recv) + (size_t)r * bytes, c->slots + (size_t)r * SLOT_BYTES, bytes, stream);
    }
  }
  if (!barrier(c)) return ncclSystemError;
  c->seq += 1;
  if (!agree) return ncclInvalidArgument;
  if (rc == ncclSuccess) g_calls[kind].fetch_add(1);
  return rc;
}

}  // namespace

extern "C" {

ncclResult_t ncclGetUniqueId(ncclUniqueId* id) {
  Mapping& m = mapping();
  if (!id) return ncclInvalidArgument;
  if (!m.base) return ncclSystemError;
  // regions from the top of the file, so ids the test makes itself (counting from 0) are never handed out here
  const uint32_t k = reinterpret_cast<Global*>(m.base)->ids_made.fetch_add(1);
  if ((size_t)k >= m.regions) return ncclSystemError;
  memset(id, 0, sizeof(*id));
  const uint32_t region = (uint32_t)(m.regions - 1 - k);
  memcpy(id->internal, &region, sizeof(region));
  return ncclSuccess;
}

ncclResult_t ncclCommInitRank(ncclComm_t* comm, int nranks, ncclUniqueId id, int rank) {
  Mapping& m = mapping();
  if (!comm || nranks < 1 || nranks > MAX_RANKS || rank < 0 || rank >= nranks) return ncclInvalidArgument;
  if (!m.base) return ncclSystemError;
  uint32_t region;
  memcpy(&region, id.internal, sizeof(region));
  if ((size_t)region >= m.regions) return ncclInvalidArgument;
  Comm* c = new (std::nothrow) Comm();
  if (!c) return ncclSystemError;
  char* base = m.base + GLOBAL_BYTES + (size_t)region * REGION_BYTES;
  c->magic = MAGIC;
  c->n = nranks;
  c->rank = rank;
  c->seq = 0;
  c->broken = false;
  c->ctl = reinterpret_cast<Control*>(base);
  // a region may have served an earlier communicator of the same ranks: start from the sense it was left in (it cannot flip
  // before this rank arrives, as a flip needs all n arrivals)
  c->sense = c->ctl->sense.load(std::memory_order_acquire);
  c->slots = base + CONTROL_BYTES;
  if (!barrier(c)) {   // as ncclCommInitRank does, wait for every rank of the communicator
    delete c;
    return ncclSystemError;
  }
  g_live.fetch_add(1);
  *comm = reinterpret_cast<ncclComm_t>(c);
  return ncclSuccess;
}

ncclResult_t ncclCommDestroy(ncclComm_t comm) {
  Comm* c = reinterpret_cast<Comm*>(comm);
  if (!c || c->magic != MAGIC) return ncclInvalidArgument;
  c->magic = 0;
  delete c;
  g_live.fetch_sub(1);
  return ncclSuccess;
}

ncclResult_t ncclAllReduce(const void* sendbuff, void* recvbuff, size_t count, ncclDataType_t datatype, ncclRedOp_t op, ncclComm_t comm,
                           hipStream_t stream) {
  return collective(1, sendbuff, recvbuff, count, datatype, op, comm, stream);
}

ncclResult_t ncclAllGather(const void* sendbuff, void* recvbuff, size_t sendcount, ncclDataType_t datatype, ncclComm_t comm, hipStream_t stream) {
  return collective(2, sendbuff, recvbuff, sendcount, datatype, ncclSum, comm, stream);
}

const char* ncclGetErrorString(ncclResult_t result) {
  switch (result) {
    case ncclSuccess: return "no error";
    case ncclSystemError: return "loopback: unhandled system error (a rank did not arrive before the deadline, or no meeting file)";
    case ncclInvalidArgument: return "loopback: invalid argument (unsupported type or operation, payload larger than a slot, or the ranks disagree)";
    case ncclUnhandledCudaError: return "loopback: a HIP call failed";
    default: return "loopback: error";
  }
}

// communicators created and not yet destroyed in this process
int loopback_live_comms() { return g_live.load(); }

// collectives served in this process: which = 1 all-reduces, 2 all-gathers
long loopback_calls(int which) { return (which == 1 || which == 2) ? g_calls[which].load() : -1; }

// bytes a rank can contribute to one collective
long loopback_slot_bytes() { return (long)SLOT_BYTES; }

}  // extern "C"
