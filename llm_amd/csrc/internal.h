// internal.h — private seam between the host-side ggml core (ggml_core.cpp) and the MI355X backend
// (hip_backend.hip).  Not part of the C ABI.
#pragma once
#include <stddef.h>

#include "ggml_hip.h"

// ggml_flash_attn keeps all scores of a query row in LDS (kernels/flash_attn.h), so the row length M is bounded by the 160 KB of
// a CU.  The kernels ask for at most FLASH_ATTN_LDS_BYTES of dynamic LDS (the 10 KB left are the margin k_p_attn keeps too).
//   one row per workgroup: 256 bytes of reduction scratch + 4 D bytes of q + 4 M bytes of scores
//   32 / 16 rows per workgroup (the MFMA kernel): rows of ((M rounded up to 64) * 4 + 16) bytes
// ggml_flash_attn rejects D > FLASH_ATTN_MAX_D and M > FLASH_ATTN_MAX_KEYS while the graph is built; rows of more than
// FLASH_ATTN_MAX_KEYS_TILE keys run one row per workgroup whatever their head size.
#define FLASH_ATTN_LDS_BYTES (150 * 1024)
#define FLASH_ATTN_MAX_D 1024
#define FLASH_ATTN_MAX_KEYS ((FLASH_ATTN_LDS_BYTES - 256 - 4 * FLASH_ATTN_MAX_D) / 4 / 64 * 64)  /* 37312 */
#define FLASH_ATTN_MAX_KEYS_TILE ((FLASH_ATTN_LDS_BYTES / 16 - 16) / 4 / 64 * 64)                /* 2368 */

extern "C" {
// Every ggml context buffer and every scratch buffer handed to ggml_set_scratch is an "arena": host
// memory whose tensors get a device mirror at the same offset inside a lazily created device shadow.
void ggml_hip_internal_register_arena(void *host_base, size_t size, int is_scratch);
void ggml_hip_internal_unregister_arena(void *host_base);
// Executes a whole cgraph on the device (called by ggml_graph_compute).
void ggml_hip_internal_graph_compute(struct ggml_cgraph *cgraph);
}
