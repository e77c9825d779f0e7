// transformer_plan.cpp — transformer_plan.h's pure functions.
#include "transformer_plan.h"

namespace ftk {

const char *transformer_refusal_name(TransformerRefusal r) {
    switch (r) {
        case TransformerRefusal::None: return "none";
        case TransformerRefusal::Rows: return "rows";
        case TransformerRefusal::Dim: return "dim";
        case TransformerRefusal::Heads: return "heads";
        case TransformerRefusal::HeadDim: return "head_dim";
    }
    return "?";
}

namespace {

uint32_t tiles(int64_t n, int64_t per) { return (uint32_t)((n + per - 1) / per); }

// The limits, and the attention part of a plan: rows0 / rows1 are the query counts of the launch's two problems.
TransformerPlan attention_part(int32_t rows0, int32_t rows1, int32_t dim, int32_t heads, int32_t aligned16, int problems) {
    TransformerPlan p{};
    if (rows0 < 1 || rows1 < 1 || rows0 > kTransformerMaxRows || rows1 > kTransformerMaxRows) {
        p.refused = TransformerRefusal::Rows;
        return p;
    }
    if (dim < 1 || dim > kTransformerMaxDim) {
        p.refused = TransformerRefusal::Dim;
        return p;
    }
    if (heads < 1 || dim % heads != 0) {
        p.refused = TransformerRefusal::Heads;
        return p;
    }
    const int32_t dh = dim / heads;
    if (dh % 2 != 0 || dh < 2 || dh > kTransformerMaxHeadDim) {
        p.refused = TransformerRefusal::HeadDim;
        return p;
    }
    p.refused = TransformerRefusal::None;
    p.head_dim = dh;
    p.vec_linear = (dim % 4 == 0 && aligned16 != 0) ? 1 : 0;
    p.vec_attn = (p.vec_linear && dh % 4 == 0) ? 1 : 0;
    const int32_t most = rows0 > rows1 ? rows0 : rows1;
    const int32_t whole = dh <= 32 ? 1 : (dh <= 64 ? 2 : 4);
    p.attn_grid_x = tiles(most, 32);
    p.attn_out_tiles = (int64_t)p.attn_grid_x * heads * problems >= kAttnFillWaves ? whole : 1;
    p.attn_grid_y = (uint32_t)heads * tiles(dh, 32 * p.attn_out_tiles);
    p.attn_grid_z = (uint32_t)problems;
    return p;
}

}  // namespace

LinearPlan linear_plan(int32_t rows, int32_t in_dim, int32_t out_dim, int32_t aligned16) {
    LinearPlan p{};
    if (rows < 1 || rows > kTransformerMaxRows) {
        p.refused = TransformerRefusal::Rows;
        return p;
    }
    if (in_dim < 1 || in_dim > kTransformerMaxDim || out_dim < 1 || out_dim > kTransformerMaxDim) {
        p.refused = TransformerRefusal::Dim;
        return p;
    }
    p.refused = TransformerRefusal::None;
    p.vec = (in_dim % 4 == 0 && aligned16 != 0) ? 1 : 0;
    p.grid_x = tiles(rows, kLinearTileRows);
    p.grid_y = tiles(out_dim, kLinearTileCols);
    return p;
}

TransformerPlan attention_plan(int32_t rows_q, int32_t rows_k, int32_t heads, int32_t head_dim, int32_t aligned16) {
    if (heads < 1 || heads > kTransformerMaxDim || head_dim < 1 || head_dim > kTransformerMaxDim) {
        TransformerPlan p{};
        p.refused = heads < 1 || heads > kTransformerMaxDim ? TransformerRefusal::Heads : TransformerRefusal::HeadDim;
        return p;
    }
    TransformerPlan p = attention_part(rows_q, rows_k, heads * head_dim, heads, aligned16, 1);
    if (p.refused == TransformerRefusal::None) {
        p.attn_grid_x = tiles(rows_q, 32);
        p.launches = 1;
    }
    return p;
}

TransformerPlan transformer_plan(const TransformerPlanInput &in) {
    TransformerPlan p = attention_part(in.rows0, in.rows1, in.dim, in.heads, in.aligned16, 2);
    if (p.refused != TransformerRefusal::None) {
        return p;
    }
    const size_t r = (size_t)in.rows0 + (size_t)in.rows1, d = (size_t)in.dim;
    p.linear_grid_x = tiles((int64_t)r, kLinearTileRows);
    p.grid_y_d = tiles(in.dim, kLinearTileCols);
    p.grid_y_2d = tiles(2 * in.dim, kLinearTileCols);
    p.grid_y_3d = tiles(3 * in.dim, kLinearTileCols);
    p.norm_blocks = (uint32_t)r;
    p.launches = 12;
    ftk_layout16 ws;  // cannot wrap: R D <= 2^23
    p.qkv = ws.take<float>(3 * r * d);
    p.ctx = ws.take<float>(r * d);
    p.msg = ws.take<float>(r * d);
    p.hidden = ws.take<float>(2 * r * d);
    p.x1 = ws.take<float>(r * d);
    p.bytes = ws.bytes();
    size_t at = 0;
    for (int block = 0; block < 2; ++block) {
        size_t *w = block == 0 ? p.w_self : p.w_cross;
        const size_t in_outs = block == 0 ? 3 * d : 2 * d;
        const size_t sizes[10] = {in_outs * d, in_outs, d * d, d, 4 * d * d, 2 * d, 2 * d, 2 * d, 2 * d * d, d};
        for (int k = 0; k < 10; ++k) {
            w[k] = at;
            at += sizes[k];
        }
    }
    p.weight_floats = at;
    return p;
}

}  // namespace ftk
