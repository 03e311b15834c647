// Host side of the persistent sweeps' contract (decoder_ws.h: SweepKernel): the one place that owns each kernel's option and
// first-use state, the tuning options of their waits and the residency check.  The state ints are plain ints, as they always were:
// a mutex around the first-use check would go into may_run / settle.
#include "decoder_ws.h"
#include "sweep_sync.h"

SweepKernel g_sweep_kernels[3] = {{1, -1, "persistent decode"}, {1, -1, "persistent training rollout"}, {1, -1, "persistent BPTT sweep"}};
int g_poll_sleep = 0;
int g_poll_stagger = 0;
int g_persistent_spin = 1 << 21;

bool stream_capturing(hipStream_t s) {
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(s, &cap) != hipSuccess) cap = hipStreamCaptureStatusActive;   // a failed query must not read as "not capturing"
  return cap != hipStreamCaptureStatusNone;
}

bool SweepKernel::may_run(hipStream_t s) const { return enabled && state != 0 && (state == 1 || !stream_capturing(s)); }

int SweepKernel::settle(hipStream_t s, const unsigned* errword, bool* ok) {
  *ok = state == 1;
  if (*ok) return 0;
  unsigned err = 1;
  ZCHECK(hipStreamSynchronize(s) == hipSuccess, "%s: stream sync failed", what);
  ZCHECK(hipMemcpy(&err, errword, sizeof(err), hipMemcpyDeviceToHost) == hipSuccess, "%s: error word copy failed", what);
  state = err == 0;
  *ok = err == 0;
  return 0;
}

SweepSync sweep_sync_args(unsigned* cnt, unsigned* err, unsigned* status) {
  return SweepSync{cnt, err, status, (unsigned)g_persistent_spin, cnt ? (unsigned)g_poll_sleep : 0u, cnt ? (unsigned)g_poll_stagger : 0u};
}

int require_cus(int n, const char* what) {
  int dev = 0, ncu = 0;
  ZCHECK(hipGetDevice(&dev) == hipSuccess, "hipGetDevice failed");
  ZCHECK(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess, "device query failed");
  ZCHECK(ncu >= n, "%s needs %d CUs (device has %d)", what, n, ncu);
  return 0;
}
