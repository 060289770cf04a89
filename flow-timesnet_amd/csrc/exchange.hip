// Host side of the peer exchanges of a sharded run (include/flowtimes.h): the IPC buffer lifecycle shared by the [F]
// batch-sum exchange (FtnExchange; written by spectrum.hip's k_colsum, read by the finalize workgroup of
// ftn_finalize.h) and the row exchange (FtnRowExchange, rowx.hip), and the [F] exchange's layout queries.
#include <string.h>
#include "ftn_exchange.h"

// ---------------------------------------------------------------- IPC buffer lifecycle
int ftn_ipc_alloc(size_t n, bool allow_cached_fallback, const char* what, void** buf_out, void* handle64_out) {
  static_assert(sizeof(hipIpcMemHandle_t) == 64, "IPC handle size");
  void* p = nullptr;
  hipError_t e = hipExtMallocWithFlags(&p, n, hipDeviceMallocUncached);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    if (!allow_cached_fallback) {
      ftn_set_error("%s: uncached allocation of %zu bytes failed: %s", what, n, hipGetErrorString(e));
      return (int)e;
    }
    // (the kernels of that exchange use system-scope loads / stores either way)
    p = nullptr;
    e = hipMalloc(&p, n);
  }
  if (e == hipSuccess) e = hipMemset(p, 0, n);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipIpcGetMemHandle((hipIpcMemHandle_t*)handle64_out, p);
  if (e != hipSuccess) {
    ftn_set_error("%s: %s", what, hipGetErrorString(e));
    if (p) (void)hipFree(p);
    return (int)e;
  }
  *buf_out = p;
  return 0;
}
int ftn_ipc_open(const char* what, const char* err, const void* handle64, void** mapped_out) {
  FTN_CHECK_ARG(handle64 && mapped_out, "%s: null pointer", what);
  hipIpcMemHandle_t h;
  memcpy(&h, handle64, sizeof(h));
  hipError_t e = hipIpcOpenMemHandle(mapped_out, h, hipIpcMemLazyEnablePeerAccess);
  if (e != hipSuccess) { ftn_set_error("%s: %s", err, hipGetErrorString(e)); return (int)e; }
  return 0;
}
int ftn_ipc_close(const char* err, void* mapped) {
  hipError_t e = mapped ? hipIpcCloseMemHandle(mapped) : hipSuccess;
  if (e != hipSuccess) { ftn_set_error("%s: %s", err, hipGetErrorString(e)); return (int)e; }
  return 0;
}
int ftn_ipc_free(const char* err, void* buf) {
  hipError_t e = buf ? hipFree(buf) : hipSuccess;
  if (e != hipSuccess) { ftn_set_error("%s: %s", err, hipGetErrorString(e)); return (int)e; }
  return 0;
}

// ---------------------------------------------------------------- the [F] batch-sum exchange
extern "C" size_t ftn_exchange_bytes(int world, int F_cap) {
  if (world < 1 || world > FTN_XCHG_MAXWORLD || F_cap < 2 || F_cap > 32 * FTN_XCHG_NBLK) return 0;
  return 2 * ftn_xchg_half_bytes(world, F_cap) + 256;           // two halves + the error word's line
}

bool ftn_xch_ok(const FtnExchange* x, int F) {
  return x->world >= 1 && x->world <= FTN_XCHG_MAXWORLD && x->rank >= 0 && x->rank < x->world &&
         (x->mode == 1 || (x->mode == 0 && x->seq > 0)) && F <= x->F_cap && x->F_cap <= 32 * FTN_XCHG_NBLK &&
         x->slots[x->rank] != nullptr;
}
int* ftn_xch_err_word(const FtnExchange* x) {
  return (int*)((char*)x->slots[x->rank] + 2 * ftn_xchg_half_bytes(x->world, x->F_cap));
}
void ftn_xch_fill(const FtnExchange* x, int F, FinalizeArgs* fa) {
  char* mine = (char*)x->slots[x->rank];
  fa->psum = (const double*)mine;
  fa->nparts = x->world;
  fa->psum_stride = x->F_cap;
  fa->ready = (const unsigned long long*)(mine + ftn_xchg_flags_off(x->world, x->F_cap));
  fa->ready_seq = x->seq;
  fa->ready_n = (F + 31) / 32;
  fa->xerr = ftn_xch_err_word(x);
  fa->xctr = ftn_xch_counter(x);
  fa->xhalf = ftn_xchg_half_bytes(x->world, x->F_cap);
}

extern "C" int ftn_exchange_alloc(int world, int F_cap, void** buf_out, void* handle64_out) {
  const size_t n = ftn_exchange_bytes(world, F_cap);
  FTN_CHECK_ARG(n > 0 && buf_out && handle64_out, "ftn_exchange_alloc: world=%d F_cap=%d", world, F_cap);
  return ftn_ipc_alloc(n, true, "ftn_exchange_alloc", buf_out, handle64_out);
}
extern "C" int ftn_exchange_open(const void* handle64, void** mapped_out) {
  return ftn_ipc_open("ftn_exchange_open", "hipIpcOpenMemHandle", handle64, mapped_out);
}
extern "C" int ftn_exchange_close(void* mapped) { return ftn_ipc_close("hipIpcCloseMemHandle", mapped); }
extern "C" int ftn_exchange_free(void* buf) { return ftn_ipc_free("hipFree", buf); }

extern "C" size_t ftn_exchange_counter_offset(int world, int F_cap) {
  return ftn_exchange_bytes(world, F_cap) > 0 ? ftn_xchg_counter_off(world, F_cap) : 0;
}

extern "C" int64_t ftn_exchange_calls(const FtnExchange* xch, void* stream) {
  FTN_CHECK_ARG(xch && xch->world >= 1 && xch->world <= FTN_XCHG_MAXWORLD && xch->rank >= 0 && xch->rank < xch->world &&
                xch->slots[xch->rank] && xch->mode == 1, "ftn_exchange_calls: bad exchange (or not mode 1)");
  unsigned long long v = 0;
  hipError_t e = hipMemcpyAsync(&v, ftn_xch_counter(xch), sizeof(v), hipMemcpyDeviceToHost, (hipStream_t)stream);
  if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
  if (e != hipSuccess) { ftn_set_error("ftn_exchange_calls: %s", hipGetErrorString(e)); return -1; }
  return (int64_t)v;
}

extern "C" int ftn_exchange_error(const FtnExchange* xch, void* stream) {
  FTN_CHECK_ARG(xch && xch->world >= 1 && xch->world <= FTN_XCHG_MAXWORLD && xch->rank >= 0 && xch->rank < xch->world &&
                xch->slots[xch->rank], "ftn_exchange_error: bad exchange");
  int v = 0;
  hipError_t e = hipMemcpyAsync(&v, ftn_xch_err_word(xch), sizeof(int), hipMemcpyDeviceToHost, (hipStream_t)stream);
  if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
  if (e != hipSuccess) { ftn_set_error("ftn_exchange_error: %s", hipGetErrorString(e)); return -(int)e - 1000; }
  return v;
}
