// Host-side interface of hash.hip (shared with the binding TU);
// the definitions there carry the argument contracts.
#pragma once

#include <hip/hip_runtime.h>

#include "common.h"

void launch_hash_touch(const long* rows, long* last_used, long n,
                       long capacity, long step, hipStream_t stream);
void launch_hash_compact_flags(const bool* keep, const long* size, int* flags,
                               long* old_size, long capacity,
                               hipStream_t stream);
void launch_hash_compact_move(const int* flags, const long* incl,
                              const long* old_size, long* holes, long* movers,
                              void* const* bases, const int* row_bytes,
                              const int* elem_bytes, int count,
                              long* row_keys, long* last_used, long* size,
                              long* evicted, long capacity,
                              hipStream_t stream);
void launch_hash_find(const long* keys, const long* slot_keys,
                      const long* slot_rows, long* rows, long n, long H,
                      hipStream_t stream);
void launch_hash_lookup(const long* keys, const long* slot_keys,
                        const long* slot_rows, long* rows, long* skeys,
                        long* spos, int* flags, long n, long H, long S,
                        hipStream_t stream);
void launch_hash_admit(const long* keys, const int* flags, int* counters,
                       int* pass, long* filtered, long n, long width,
                       long admit_after, hipStream_t stream);
void launch_hash_insert(const long* keys, const int* flags, const long* incl,
                        long* slot_keys, long* slot_rows, long* row_keys,
                        long* size, long* dropped, long* rows, bool* is_new,
                        long n, long H, long capacity, hipStream_t stream);
void launch_hash_rebuild(const long* row_keys, const long* size,
                         long* slot_keys, long* slot_rows, long H,
                         long capacity, hipStream_t stream);
void launch_hash_gather(const long* keys, const long* slot_keys,
                        const long* slot_rows, const bf16_t* table,
                        bf16_t* out, long n, long H, long V, int D,
                        hipStream_t stream);
void launch_hash_init_rows(const long* keys, const long* rows,
                           const bool* is_new, float* master, bf16_t* shadow,
                           float* s1, float* s2, long n, long V, int D,
                           long seed, long key_mul, long key_add, float scale,
                           hipStream_t stream);
void launch_hash_gather_init(const long* keys, const long* slot_keys,
                             const long* slot_rows, const bf16_t* table,
                             bf16_t* out, long* last_used, long n, long H,
                             long V, int D, long stamps, long step, long seed,
                             long key_mul, long key_add, float scale,
                             hipStream_t stream);
void launch_hash_embedding_bag(const long* keys, const long* slot_keys,
                               const long* slot_rows, const bf16_t* table,
                               const long* offsets, const float* weights,
                               void* out, bool o_bf16, long* last_used,
                               long B, long n, long H, long V, int D,
                               bool mean, long stamps, long step,
                               bool has_init, long seed, long key_mul,
                               long key_add, float scale,
                               hipStream_t stream);
