// MCPNet's sizes and the layout of its packed weights (lrg_mcp_pack_weights), shared by the inference kernel (lrg_mcpnet.hip) and
// the training forward (lrg_mcpnet_train.hip): both read one packed buffer.
#pragma once
#include "lrg_common.h"

#define MCP_K LRG_MCP_NEIGHBORS      // 50 rows per point
#define MCP_H 200
#define MCP_E 10
#define MCP_NT 7                     // 32-column tiles of layer 2
#define MCP_KG 25                    // float4 k-groups of layer 2 (100 k-steps of two)
#define MCP_FD 5                     // depth of the weight ring (groups)
#define MCP_OFF_K1 0                 // [200][8]: K1[0..5][c], b1[c], b2[c]
#define MCP_OFF_K2 1600              // [7][25][64] float4: lane l, component q of group g of tile t = K2[8 g + 2 q + (l >> 5)][32 t + (l & 31)]
#define MCP_OFF_K3 46400             // [204][200]
#define MCP_OFF_B3 87200             // [200]
#define MCP_OFF_K4 87400             // [200][10]
#define MCP_OFF_B4 89400             // [16]
#define MCP_PACKED 89416

typedef float f32x16 __attribute__((ext_vector_type(16)));
