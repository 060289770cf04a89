// Host side of the two peer exchanges (exchange.hip): what the other units need of the [F] batch-sum exchange
// (FtnExchange: k_colsum writes it, the finalize workgroup waits on it) and the IPC buffer lifecycle it shares with
// the row exchange of rowx.hip.  Library-internal: none of this is part of the C ABI.
#pragma once
#include "ftn_common.h"
#include "ftn_finalize.h"

// mode 0 needs the host's sequence number (> 0); mode 1 keeps it in the buffer's call counter
bool ftn_xch_ok(const FtnExchange* x, int F);
int* ftn_xch_err_word(const FtnExchange* x);
// the finalize side of an exchange: psum rows = the world slots of this rank's own buffer (the kernel picks the half)
void ftn_xch_fill(const FtnExchange* x, int F, FinalizeArgs* fa);

static inline bool ftn_xch_mapped(const FtnExchange* x) {
  for (int r = 0; r < x->world; ++r)
    if (x->slots[r] == nullptr) return false;
  return true;
}
static inline unsigned long long* ftn_xch_counter(const FtnExchange* x) {
  return x->mode == 1 ? (unsigned long long*)((char*)x->slots[x->rank] + ftn_xchg_counter_off(x->world, x->F_cap))
                      : nullptr;
}

// One rank's buffer of n bytes: uncached device memory (what RCCL uses for words that GPUs exchange inside running
// kernels: every access goes to memory, whichever GPU issues it), zeroed, its own allocation - which is what an IPC
// handle names - and exported as a 64-byte handle the other ranks open.  allow_cached_fallback: plain hipMalloc where
// the runtime offers no uncached memory.  `what` / `err` prefix the error text (the caller's name, or the runtime
// call's where the [F] exchange has always reported that).
#define FTN_INTERNAL __attribute__((visibility("hidden")))
FTN_INTERNAL int ftn_ipc_alloc(size_t n, bool allow_cached_fallback, const char* what, void** buf_out, void* handle64_out);
FTN_INTERNAL int ftn_ipc_open(const char* what, const char* err, const void* handle64, void** mapped_out);
FTN_INTERNAL int ftn_ipc_close(const char* err, void* mapped);
FTN_INTERNAL int ftn_ipc_free(const char* err, void* buf);
