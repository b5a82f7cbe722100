// loopback_rccl_driver.cpp — stand-alone check of tests/host_ref/loopback_rccl.cpp in its host-buffer build
// (-DLOOPBACK_HOST_BUFFERS: the "device" buffers are host memory, no HIP call is made).  Compiled together with that file;
// forks the ranks itself, one group of processes per case, and waits for every one of them.
//   usage: loopback_rccl_driver <directory for the meeting file>
// Exit status 0 and a last line "ok" when every case passed.  Built plain and with -fsanitize=address,undefined by
// tests/test_multirank_loopback.py.
#include <rccl/rccl.h>

#include <fcntl.h>
#include <signal.h>
#include <sys/wait.h>
#include <time.h>
#include <unistd.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

extern "C" int loopback_live_comms();
extern "C" long loopback_calls(int which);
extern "C" long loopback_slot_bytes();

namespace {

constexpr size_t FILE_BYTES = 4096 + 6 * (size_t(2) << 20);

#define CHECK(cond)                                                                      \
  do {                                                                                   \
    if (!(cond)) {                                                                       \
      fprintf(stderr, "rank %d: line %d: CHECK(%s) failed\n", g_rank, __LINE__, #cond); \
      return 1;                                                                          \
    }                                                                                    \
  } while (0)

int g_rank = -1;

double now() {
  timespec t;
  clock_gettime(CLOCK_MONOTONIC, &t);
  return (double)t.tv_sec + 1e-9 * (double)t.tv_nsec;
}

ncclUniqueId id_of_region(uint32_t region) {
  ncclUniqueId id;
  memset(&id, 0x5a, sizeof(id));   // (everything after the first four bytes is opaque)
  memcpy(id.internal, &region, sizeof(region));
  return id;
}

double val(int rank, size_t i) { return (rank + 1) * 0.1 + (double)i * (rank % 2 ? -1.7 : 0.3) + 1e-9 * rank; }

// sum and max all-reduce, all-gather of double and float, each out of place and in place; rank order; the counters
int case_collectives(int rank, int n) {
  ncclComm_t comm = nullptr;
  CHECK(loopback_live_comms() == 0);
  CHECK(ncclCommInitRank(&comm, n, id_of_region(0), rank) == ncclSuccess);
  CHECK(loopback_live_comms() == 1);
  const size_t cnt = 1031;
  std::vector<double> mine(cnt), out(cnt), want(cnt);
  for (int pass = 0; pass < 4; ++pass) {
    const bool in_place = pass & 1;
    const ncclRedOp_t op = pass < 2 ? ncclSum : ncclMax;
    for (size_t i = 0; i < cnt; ++i) {
      mine[i] = val(rank, i);
      double acc = val(0, i);
      for (int r = 1; r < n; ++r) acc = op == ncclSum ? acc + val(r, i) : (acc > val(r, i) ? acc : val(r, i));   // rank order
      want[i] = acc;
    }
    double* recv = in_place ? mine.data() : out.data();
    CHECK(ncclAllReduce(mine.data(), recv, cnt, ncclDouble, op, comm, nullptr) == ncclSuccess);
    CHECK(memcmp(recv, want.data(), cnt * sizeof(double)) == 0);
    if (!in_place)
      for (size_t i = 0; i < cnt; ++i) CHECK(mine[i] == val(rank, i));   // the send buffer is left alone
  }
  for (int pass = 0; pass < 2; ++pass) {   // all-gather of double: block r of the result is rank r's buffer
    const bool in_place = pass & 1;
    std::vector<double> all(cnt * n, -1.0), send(cnt);
    for (size_t i = 0; i < cnt; ++i) send[i] = val(rank, i);
    const double* s = send.data();
    if (in_place) {
      memcpy(all.data() + cnt * rank, send.data(), cnt * sizeof(double));
      s = all.data() + cnt * rank;
    }
    CHECK(ncclAllGather(s, all.data(), cnt, ncclDouble, comm, nullptr) == ncclSuccess);
    for (int r = 0; r < n; ++r)
      for (size_t i = 0; i < cnt; ++i) CHECK(all[cnt * r + i] == val(r, i));
  }
  for (int pass = 0; pass < 2; ++pass) {   // and of float
    const bool in_place = pass & 1;
    const size_t c7 = 7;
    std::vector<float> all(c7 * n, -1.0f), send(c7);
    for (size_t i = 0; i < c7; ++i) send[i] = (float)val(rank, i);
    const float* s = send.data();
    if (in_place) {
      memcpy(all.data() + c7 * rank, send.data(), c7 * sizeof(float));
      s = all.data() + c7 * rank;
    }
    CHECK(ncclAllGather(s, all.data(), c7, ncclFloat, comm, nullptr) == ncclSuccess);
    for (int r = 0; r < n; ++r)
      for (size_t i = 0; i < c7; ++i) CHECK(all[c7 * r + i] == (float)val(r, i));
  }
  CHECK(loopback_calls(1) == 4 && loopback_calls(2) == 4);
  CHECK(ncclCommDestroy(comm) == ncclSuccess);
  CHECK(loopback_live_comms() == 0);
  return 0;
}

// what the engine does not use is refused on every rank, and the communicator stays usable afterwards
int case_refusals(int rank, int n) {
  ncclComm_t comm = nullptr;
  CHECK(ncclCommInitRank(&comm, n, id_of_region(1), rank) == ncclSuccess);
  double a[8] = {1, 2, 3, 4, 5, 6, 7, 8}, b[8 * 8];
  // a count mismatch between the ranks
  CHECK(ncclAllReduce(a, b, rank == n - 1 ? 5 : 4, ncclDouble, ncclSum, comm, nullptr) == ncclInvalidArgument);
  CHECK(ncclAllGather(a, b, rank == 0 ? 2 : 3, ncclDouble, comm, nullptr) == ncclInvalidArgument);
  // types and operations outside the supported set
  CHECK(ncclAllReduce(a, b, 4, ncclFloat, ncclSum, comm, nullptr) == ncclInvalidArgument);
  CHECK(ncclAllReduce(a, b, 4, ncclDouble, ncclProd, comm, nullptr) == ncclInvalidArgument);
  CHECK(ncclAllReduce(a, b, 4, ncclDouble, ncclMin, comm, nullptr) == ncclInvalidArgument);
  CHECK(ncclAllGather(a, b, 4, ncclInt32, comm, nullptr) == ncclInvalidArgument);
  // one rank disagrees about the operation
  CHECK(ncclAllReduce(a, b, 4, ncclDouble, rank == 1 ? ncclMax : ncclSum, comm, nullptr) == ncclInvalidArgument);
  // a payload larger than a slot: refused before the buffer is read
  CHECK(ncclAllGather(a, b, (size_t)loopback_slot_bytes() / 8 + 1, ncclDouble, comm, nullptr) == ncclInvalidArgument);
  CHECK(ncclAllReduce(a, b, (size_t)loopback_slot_bytes() / 8 + 1, ncclDouble, ncclSum, comm, nullptr) == ncclInvalidArgument);
  CHECK(loopback_calls(1) == 0 && loopback_calls(2) == 0);
  // the ranks are still in step
  CHECK(ncclAllReduce(a, b, 8, ncclDouble, ncclSum, comm, nullptr) == ncclSuccess);
  for (int i = 0; i < 8; ++i) CHECK(b[i] == n * a[i]);
  CHECK(loopback_calls(1) == 1);
  CHECK(ncclCommDestroy(comm) == ncclSuccess);
  CHECK(ncclCommDestroy(nullptr) == ncclInvalidArgument);
  CHECK(loopback_live_comms() == 0);
  // ids outside the file, rank outside the communicator
  CHECK(ncclCommInitRank(&comm, n, id_of_region(1000), rank) == ncclInvalidArgument);
  CHECK(ncclCommInitRank(&comm, n, id_of_region(1), n) == ncclInvalidArgument);
  return 0;
}

// three ranks announced, two present (deadline 1 s): ncclCommInitRank gives up with ncclSystemError
int case_absent_at_init(int rank, int n) {
  ncclComm_t comm = nullptr;
  const double t0 = now();
  CHECK(ncclCommInitRank(&comm, n + 1, id_of_region(2), rank) == ncclSystemError);
  CHECK(now() - t0 < 5.0);
  CHECK(comm == nullptr && loopback_live_comms() == 0);
  return 0;
}

// a rank that leaves before a collective: the others give up with ncclSystemError, and the communicator stays refused
int case_absent_at_collective(int rank, int n) {
  ncclComm_t comm = nullptr;
  CHECK(ncclCommInitRank(&comm, n, id_of_region(3), rank) == ncclSuccess);
  double a[4] = {1, 2, 3, 4};
  CHECK(ncclAllReduce(a, a, 4, ncclDouble, ncclSum, comm, nullptr) == ncclSuccess);
  if (rank != n - 1) {
    const double t0 = now();
    CHECK(ncclAllReduce(a, a, 4, ncclDouble, ncclSum, comm, nullptr) == ncclSystemError);
    CHECK(now() - t0 < 5.0);
    CHECK(ncclAllGather(a, a, 1, ncclDouble, comm, nullptr) == ncclSystemError);   // broken: no second wait
    CHECK(now() - t0 < 5.0);
  }
  CHECK(ncclCommDestroy(comm) == ncclSuccess);
  CHECK(loopback_live_comms() == 0);
  return 0;
}

// the ids ncclGetUniqueId hands out are distinct regions, away from the ones made by hand
int case_unique_ids(int rank, int n) {
  (void)rank;
  (void)n;
  ncclUniqueId a, b;
  CHECK(ncclGetUniqueId(&a) == ncclSuccess && ncclGetUniqueId(&b) == ncclSuccess);
  uint32_t ra, rb;
  memcpy(&ra, a.internal, 4);
  memcpy(&rb, b.internal, 4);
  CHECK(ra != rb && ra >= 4 && rb >= 4);
  ncclComm_t comm = nullptr;   // a communicator of one rank: every collective is a copy
  CHECK(ncclCommInitRank(&comm, 1, a, 0) == ncclSuccess);
  double x[3] = {1.5, -2.5, 3.5}, y[3] = {0, 0, 0};
  CHECK(ncclAllReduce(x, y, 3, ncclDouble, ncclMax, comm, nullptr) == ncclSuccess);
  CHECK(memcmp(x, y, sizeof(x)) == 0);
  CHECK(ncclAllGather(x, x, 3, ncclDouble, comm, nullptr) == ncclSuccess);
  CHECK(ncclCommDestroy(comm) == ncclSuccess);
  CHECK(std::string(ncclGetErrorString(ncclSystemError)).find("deadline") != std::string::npos);
  return 0;
}

struct Case {
  const char* name;
  int (*fn)(int, int);
  int procs, n;
};

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: %s <directory>\n", argv[0]);
    return 2;
  }
  const std::string path = std::string(argv[1]) + "/loopback_driver.meet";
  const int fd = open(path.c_str(), O_RDWR | O_CREAT | O_TRUNC, 0600);
  if (fd < 0 || ftruncate(fd, (off_t)FILE_BYTES) != 0) {
    perror("meeting file");
    return 2;
  }
  close(fd);
  setenv("LOOPBACK_RCCL_FILE", path.c_str(), 1);
  setenv("LOOPBACK_RCCL_DEADLINE_S", "1", 1);
  const Case cases[] = {{"collectives", case_collectives, 3, 3},
                        {"refusals", case_refusals, 3, 3},
                        {"absent_at_init", case_absent_at_init, 2, 2},
                        {"absent_at_collective", case_absent_at_collective, 3, 3},
                        {"unique_ids", case_unique_ids, 1, 1}};
  int failed = 0;
  for (const Case& c : cases) {
    const double t0 = now();
    std::vector<pid_t> kids;
    for (int r = 0; r < c.procs; ++r) {
      fflush(nullptr);
      const pid_t p = fork();
      if (p < 0) {
        perror("fork");
        return 2;
      }
      if (p == 0) {
        g_rank = r;
        alarm(30);   // a child that is stuck anyway ends by SIGALRM: nothing is left behind
        const int rc = c.fn(r, c.n);
        fflush(nullptr);
        _exit(rc);
      }
      kids.push_back(p);
    }
    bool ok = true;
    for (pid_t p : kids) {
      int st = 0;
      if (waitpid(p, &st, 0) != p || !WIFEXITED(st) || WEXITSTATUS(st) != 0) ok = false;
    }
    for (pid_t p : kids) ok = ok && kill(p, 0) != 0;   // every child was reaped: none is left
    printf("%-22s %s  (%.2f s)\n", c.name, ok ? "ok" : "FAILED", now() - t0);
    failed += ok ? 0 : 1;
  }
  unlink(path.c_str());
  if (failed) {
    printf("%d case(s) failed\n", failed);
    return 1;
  }
  printf("ok\n");
  return 0;
}
