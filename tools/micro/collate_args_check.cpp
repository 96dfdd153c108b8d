// The argument checks of sgx_collate_graphs_extras (include/sgx.h) from a C++ host without a GPU: NULL and misshapen
// descriptors, every one of which must be refused before anything reaches a device.  Meant for a sanitizer build of
// the host code -- compile csrc/collate.hip and this file into one program:
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -I include -I sgracex1_amd/csrc \
//         sgracex1_amd/csrc/collate.hip -x hip tools/micro/collate_args_check.cpp -o tools/micro/collate_args_check
//   tools/micro/collate_args_check        # prints "ok", exit status 0
//
// Every call here is refused (a call that passed would launch on made-up addresses), so the program needs no device.
#include <cstdint>
#include <cstdio>

#include "sgx.h"

static int failures = 0;

#define EXPECT(call, want)                                                                  \
    do {                                                                                    \
        const int got_ = (call);                                                            \
        if (got_ != (want)) {                                                               \
            std::printf("line %d: %s = %d, expected %d\n", __LINE__, #call, got_, (want));  \
            ++failures;                                                                     \
        }                                                                                   \
    } while (0)

template <class T> static T *fake() { return reinterpret_cast<T *>(static_cast<uintptr_t>(0x1000)); }

static sgx_graph_set valid_set()
{
    sgx_graph_set s = {};
    s.n_graphs = 4, s.n_feat = 7, s.n_edges = 10;
    s.node_ptr = s.edge_ptr = s.edge_index = fake<const int32_t>();
    s.x = fake<const float>(), s.y = fake<const int64_t>();
    s.rowPtr_adj = s.columnIndex_adj = s.rowPtr_fea = s.columnIndex_fea = fake<const int32_t>();
    s.values_adj = s.values_fea = fake<const float>();
    return s;
}

static sgx_graph_batch valid_batch()
{
    sgx_graph_batch b = {};
    b.n_graphs = 2, b.n_rows = 5, b.n_edges = 6, b.nnz_adj = 6, b.nnz_fea = 5;
    b.index = b.node_off = b.edge_off = b.adj_off = b.fea_off = fake<const int32_t>();
    b.x = fake<float>(), b.edge_index = b.batch = b.y = fake<int64_t>();
    b.graph_ptr = b.rowPtr_adj = b.columnIndex_adj = b.rowPtr_fea = b.columnIndex_fea = fake<int32_t>();
    return b;
}

static sgx_collate_extra valid_extra()
{
    sgx_collate_extra x = {};
    x.rowPtr = x.columnIndex = x.entry_off = fake<const int32_t>();
    x.values = fake<const float>(), x.dead_row = fake<const uint8_t>();
    x.nnz = 11;
    x.rowPtr_out = x.columnIndex_out = fake<int32_t>();
    x.values_out[SGX_F32] = fake<void>();
    x.dead_row_out = fake<uint8_t>();
    return x;
}

int main()
{
    sgx_graph_set s = valid_set();
    sgx_graph_batch b = valid_batch();
    sgx_collate_extra xs[SGX_COLLATE_MAX_EXTRAS] = {valid_extra(), valid_extra(), valid_extra()};

    // K outside 0 .. 3 is judged first
    EXPECT(sgx_collate_graphs_extras(&s, &b, xs, SGX_COLLATE_MAX_EXTRAS + 1, nullptr), SGX_ERR_SHAPE);
    EXPECT(sgx_collate_graphs_extras(&s, &b, xs, -1, nullptr), SGX_ERR_SHAPE);
    EXPECT(sgx_collate_graphs_extras(nullptr, nullptr, nullptr, 1 << 30, nullptr), SGX_ERR_SHAPE);
    // the statuses of sgx_collate_graphs
    EXPECT(sgx_collate_graphs_extras(nullptr, &b, xs, 1, nullptr), SGX_ERR_NULL);
    EXPECT(sgx_collate_graphs_extras(&s, nullptr, xs, 1, nullptr), SGX_ERR_NULL);
    EXPECT(sgx_collate_graphs_extras(nullptr, nullptr, nullptr, 0, nullptr), SGX_ERR_NULL);
    EXPECT(sgx_collate_graphs(nullptr, nullptr, nullptr), SGX_ERR_NULL);
    {
        sgx_graph_batch bad = b;
        bad.n_graphs = 0;
        EXPECT(sgx_collate_graphs_extras(&s, &bad, xs, 3, nullptr), SGX_ERR_SHAPE);
        EXPECT(sgx_collate_graphs(&s, &bad, nullptr), SGX_ERR_SHAPE);
        bad = b, bad.nnz_fea = -1;
        EXPECT(sgx_collate_graphs_extras(&s, &bad, nullptr, 0, nullptr), SGX_ERR_SHAPE);
        bad = b, bad.graph_ptr = nullptr;
        EXPECT(sgx_collate_graphs_extras(&s, &bad, nullptr, 0, nullptr), SGX_ERR_NULL);
        bad = b, bad.x = nullptr;
        EXPECT(sgx_collate_graphs_extras(&s, &bad, xs, 2, nullptr), SGX_ERR_NULL);
        sgx_graph_set bs = s;
        bs.n_feat = 0;
        EXPECT(sgx_collate_graphs_extras(&bs, &b, xs, 1, nullptr), SGX_ERR_SHAPE);
        bs = s, bs.values_fea = nullptr;
        EXPECT(sgx_collate_graphs_extras(&bs, &b, xs, 1, nullptr), SGX_ERR_NULL);
    }
    // the extras' own
    EXPECT(sgx_collate_graphs_extras(&s, &b, nullptr, 1, nullptr), SGX_ERR_NULL);
    for (int k = 0; k < SGX_COLLATE_MAX_EXTRAS; ++k) {
        sgx_collate_extra keep = xs[k];
        xs[k].rowPtr = nullptr;
        EXPECT(sgx_collate_graphs_extras(&s, &b, xs, SGX_COLLATE_MAX_EXTRAS, nullptr), SGX_ERR_NULL);
        xs[k] = keep, xs[k].values = nullptr;
        EXPECT(sgx_collate_graphs_extras(&s, &b, xs, SGX_COLLATE_MAX_EXTRAS, nullptr), SGX_ERR_NULL);
        xs[k] = keep, xs[k].entry_off = nullptr;
        EXPECT(sgx_collate_graphs_extras(&s, &b, xs, SGX_COLLATE_MAX_EXTRAS, nullptr), SGX_ERR_NULL);
        xs[k] = keep, xs[k].nnz = -1;
        EXPECT(sgx_collate_graphs_extras(&s, &b, xs, SGX_COLLATE_MAX_EXTRAS, nullptr), SGX_ERR_SHAPE);
        xs[k] = keep, xs[k].rowPtr_out = nullptr;                       // columns without a row pointer
        EXPECT(sgx_collate_graphs_extras(&s, &b, xs, SGX_COLLATE_MAX_EXTRAS, nullptr), SGX_ERR_NULL);
        xs[k] = keep, xs[k].columnIndex_out = nullptr;                  // a written pattern needs its columns
        EXPECT(sgx_collate_graphs_extras(&s, &b, xs, SGX_COLLATE_MAX_EXTRAS, nullptr), SGX_ERR_NULL);
        xs[k] = keep, xs[k].columnIndex = nullptr;
        EXPECT(sgx_collate_graphs_extras(&s, &b, xs, SGX_COLLATE_MAX_EXTRAS, nullptr), SGX_ERR_NULL);
        xs[k] = keep, xs[k].dead_row = nullptr;                         // exactly one of the two row-byte arrays
        EXPECT(sgx_collate_graphs_extras(&s, &b, xs, SGX_COLLATE_MAX_EXTRAS, nullptr), SGX_ERR_NULL);
        xs[k] = keep, xs[k].dead_row_out = nullptr;
        EXPECT(sgx_collate_graphs_extras(&s, &b, xs, SGX_COLLATE_MAX_EXTRAS, nullptr), SGX_ERR_NULL);
        xs[k] = keep;
    }
    if (failures == 0) std::printf("ok\n");
    return failures != 0;
}
