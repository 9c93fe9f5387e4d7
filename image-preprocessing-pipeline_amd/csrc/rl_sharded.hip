// Sharded fused iteration (slab driver): mi_rl_iterate cut where the y halos of a convolution's input are refreshed, and the
// spectrum rows the shards exchange there.  Only the native FFT pipeline fuses consecutive convolutions, so every entry starts
// from sharded_native.
#include "rl_internal.h"

using namespace mi;

int mi::sharded_native(mi_rl_ctx* ctx, NativeFft** out) {
    MI_REQUIRE(ctx, "mi_rl_sharded: null context");
    MI_TRY(use_device(ctx->dev));
    *out = fusing_native(ctx);
    if (!*out) return fail(MI_ERR_UNSUPPORTED, "mi_rl_sharded: only the native FFT pipeline fuses consecutive convolutions");
    return (*out)->release_spare();   // (only the fused loop of mi_rl_iterate settles the spare S array: here it would stay for good)
}

extern "C" int mi_rl_sharded_begin(mi_rl_ctx* ctx, void* stream, const float* bl) {
    NativeFft* nf = nullptr;
    MI_TRY(sharded_native(ctx, &nf));
    MI_REQUIRE(bl, "mi_rl_sharded_begin: null pointer");
    return nf->x_forward(as_stream(stream), bl);
}

// part 0: the whole step; 1: the y/z passes and the x tiles holding rows of [a0,a1) or [b0,b1); 2: the remaining x tiles
static int sharded_step(mi_rl_ctx* ctx, void* stream, float* bl, bool update, int more, int part, const int* edges) {
    NativeFft* nf = nullptr;
    MI_TRY(sharded_native(ctx, &nf));
    MI_REQUIRE(bl, "mi_rl_sharded: null pointer");
    MI_REQUIRE(part >= 0 && part <= 2, "mi_rl_sharded: part must be 0, 1 or 2");
    TileSelect sel{};
    if (part != 0) {
        MI_REQUIRE(nf->splits(), "mi_rl_sharded: this context cannot split the x pass (mi_rl_fuses() != 2)");
        MI_TRY(check_edge_rows("mi_rl_sharded", edges, ctx->n[1]));
        sel = nf->edge_tiles(part, edges[0], edges[1], edges[2], edges[3]);
    }
    ConvEpilogue e;
    e.a = bl;
    if (part != 2) MI_TRY(nf->middle(as_stream(stream), update));
    return update ? nf->x_inverse(as_stream(stream), bl, EPI_UPDATE, e, more != 0, &sel)
                  : nf->x_inverse(as_stream(stream), nullptr, EPI_RATIO, e, true, &sel);
}

extern "C" int mi_rl_sharded_ratio(mi_rl_ctx* ctx, void* stream, const float* bl, int part, const int* edge_rows) {
    return sharded_step(ctx, stream, const_cast<float*>(bl), false, 1, part, edge_rows);
}

extern "C" int mi_rl_sharded_update(mi_rl_ctx* ctx, void* stream, float* bl, int more, int part, const int* edge_rows) {
    MI_REQUIRE(part == 0 || more, "mi_rl_sharded_update: a split step must produce the next input (more != 0)");
    return sharded_step(ctx, stream, bl, true, more, part, edge_rows);
}

extern "C" int mi_rl_set_overlap(mi_rl_ctx* ctx, int free_cus, int dynamic_tiles) {
    NativeFft* nf = nullptr;
    MI_TRY(sharded_native(ctx, &nf));
    MI_REQUIRE(free_cus >= 0 && free_cus < nf->n_cu, "mi_rl_set_overlap: free_cus must be in [0, %d)", nf->n_cu);
    nf->overlap_free_cus = free_cus;
    nf->overlap_dynamic = dynamic_tiles != 0;
    return MI_OK;
}

extern "C" int mi_rl_spectrum_rows(mi_rl_ctx* ctx, void* stream, int y0, int rows, float* buf, int dir) {
    NativeFft* nf = nullptr;
    MI_TRY(sharded_native(ctx, &nf));
    MI_REQUIRE(dir >= 0 && dir <= 2, "mi_rl_spectrum_rows: dir must be 0 (pack), 1 (unpack) or 2 (zero)");
    return nf->spectrum_rows(as_stream(stream), y0, rows, reinterpret_cast<float2*>(buf), dir);
}

extern "C" int mi_rl_spectrum_rows_z(mi_rl_ctx* ctx, void* stream, int y0, int rows, int z0, int z1, float* buf, int dir) {
    NativeFft* nf = nullptr;
    MI_TRY(sharded_native(ctx, &nf));
    MI_REQUIRE(dir >= 0 && dir <= 2, "mi_rl_spectrum_rows_z: dir must be 0 (pack), 1 (unpack) or 2 (zero)");
    MI_REQUIRE(z0 >= 0 && z0 < z1 && z1 <= ctx->n[2], "mi_rl_spectrum_rows_z: planes [%d, %d) outside [0, %d)", z0, z1, ctx->n[2]);
    return nf->spectrum_rows(as_stream(stream), y0, rows, reinterpret_cast<float2*>(buf), dir, z0, z1 - z0);
}

extern "C" int mi_rl_z_granule(mi_rl_ctx* ctx) {
    NativeFft* nf = nullptr;
    if (sharded_native(ctx, &nf) != MI_OK || !nf->splits()) return 0;
    return nf->y_z_granule();
}

// The sharded step cut into the stages of the z-chunked halo exchange (see include/mi_lsdeconv.h)
extern "C" int mi_rl_sharded_stage(mi_rl_ctx* ctx, void* stream, float* bl, int update, int stage, int z0, int z1, const int* edges) {
    NativeFft* nf = nullptr;
    MI_TRY(sharded_native(ctx, &nf));
    MI_REQUIRE(stage >= 0 && stage <= 3, "mi_rl_sharded_stage: stage must be 0 .. 3");
    MI_REQUIRE(nf->splits(), "mi_rl_sharded_stage: this context cannot split the x pass (mi_rl_fuses() != 2)");
    hipStream_t s = as_stream(stream);
    if (stage == 0) {
        MI_REQUIRE(z0 >= 0 && z0 < z1 && z1 <= ctx->n[2], "mi_rl_sharded_stage: planes [%d, %d) outside [0, %d)", z0, z1, ctx->n[2]);
        return nf->y_forward_planes(s, z0, z1 - z0);
    }
    if (stage == 1) {
        MI_TRY(nf->z_conv(s, update != 0));
        return nf->y_pass(s, true, y_route(nf->dims));
    }
    MI_REQUIRE(bl, "mi_rl_sharded_stage: null pointer");
    MI_TRY(check_edge_rows("mi_rl_sharded_stage", edges, ctx->n[1]));
    TileSelect sel = nf->edge_tiles(stage == 2 ? 1 : 2, edges[0], edges[1], edges[2], edges[3]);
    if (stage == 2) {
        MI_REQUIRE(z0 >= 0 && z0 < z1 && z1 <= ctx->n[2], "mi_rl_sharded_stage: planes [%d, %d) outside [0, %d)", z0, z1, ctx->n[2]);
        sel.z0 = z0;
        sel.nz = z1 - z0;
    }
    ConvEpilogue e;
    e.a = bl;
    return update ? nf->x_inverse(s, bl, EPI_UPDATE, e, true, &sel) : nf->x_inverse(s, nullptr, EPI_RATIO, e, true, &sel);
}
