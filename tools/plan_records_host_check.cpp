// Host-only soundness check of the launch plan's record handling, for a sanitizer build (tools/plan_records_host_check.sh):
// replays tests/golden/plan_calls.txt - the call list of tests/test_plan_records_cpu.py, fake device pointers - on a fresh plan,
// reads every entry's info after every call (so the entry vector is read across each of its reallocations), and destroys the
// plan.  Nothing is launched: no GPU is needed or touched.  Prints one line per call (return code, plan size) and per entry (the
// twelve info values); exit status 0 when the whole list was replayed.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../include/mindpose_hip.h"

struct Arg {
    long long v = 0;  // an integer or a (fake) device address; 0 = null
    mp_conv_desc d{};
    bool is_desc = false;
};

static const mp_conv_desc* D(const Arg& a) { return a.is_desc ? &a.d : nullptr; }
static float* F(const Arg& a) { return reinterpret_cast<float*>(static_cast<uintptr_t>(a.v)); }
static void* V(const Arg& a) { return reinterpret_cast<void*>(static_cast<uintptr_t>(a.v)); }
static int I(const Arg& a) { return (int)a.v; }

static int call(const std::string& fn, mp_plan* p, const std::vector<Arg>& a) {
    if (fn == "mp_plan_set_lane") return mp_plan_set_lane(p, I(a[0]));
    if (fn == "mp_plan_add_barrier") return mp_plan_add_barrier(p);
    if (fn == "mp_plan_add_conv") return mp_plan_add_conv(p, D(a[0]), F(a[1]), F(a[2]), F(a[3]), F(a[4]), F(a[5]), F(a[6]), F(a[7]));
    if (fn == "mp_plan_add_conv_variant")
        return mp_plan_add_conv_variant(p, D(a[0]), I(a[1]), F(a[2]), F(a[3]), F(a[4]), F(a[5]), F(a[6]), F(a[7]), F(a[8]));
    if (fn == "mp_plan_add_conv_winograd")
        return mp_plan_add_conv_winograd(p, D(a[0]), F(a[1]), F(a[2]), F(a[3]), F(a[4]), F(a[5]), F(a[6]), F(a[7]));
    if (fn == "mp_plan_add_deconv4x4s2_gemm") return mp_plan_add_deconv4x4s2_gemm(p, D(a[0]), F(a[1]), F(a[2]), F(a[3]), F(a[4]), F(a[5]));
    if (fn == "mp_plan_add_conv_f16")
        return mp_plan_add_conv_f16(p, D(a[0]), I(a[1]), V(a[2]), V(a[3]), F(a[4]), F(a[5]), V(a[6]), V(a[7]), V(a[8]));
    if (fn == "mp_plan_add_basicblock_f16")
        return mp_plan_add_basicblock_f16(p, V(a[0]), V(a[1]), F(a[2]), F(a[3]), V(a[4]), F(a[5]), F(a[6]), V(a[7]), I(a[8]), I(a[9]), I(a[10]),
                                          I(a[11]), I(a[12]));
    if (fn == "mp_plan_add_expand_reduce_f16")
        return mp_plan_add_expand_reduce_f16(p, V(a[0]), V(a[1]), V(a[2]), F(a[3]), F(a[4]), I(a[5]), V(a[6]), F(a[7]), F(a[8]), I(a[9]), V(a[10]),
                                             V(a[11]), I(a[12]), I(a[13]), I(a[14]), I(a[15]), I(a[16]), I(a[17]));
    if (fn == "mp_plan_add_ds_expand_reduce_f16")
        return mp_plan_add_ds_expand_reduce_f16(p, V(a[0]), V(a[1]), V(a[2]), F(a[3]), F(a[4]), V(a[5]), F(a[6]), F(a[7]), I(a[8]), V(a[9]), F(a[10]),
                                                F(a[11]), I(a[12]), V(a[13]), V(a[14]), I(a[15]), I(a[16]), I(a[17]), I(a[18]), I(a[19]), I(a[20]));
    if (fn == "mp_plan_add_dual_pw_f16")
        return mp_plan_add_dual_pw_f16(p, V(a[0]), V(a[1]), F(a[2]), F(a[3]), I(a[4]), V(a[5]), F(a[6]), F(a[7]), I(a[8]), V(a[9]), V(a[10]), I(a[11]),
                                       I(a[12]), I(a[13]), I(a[14]), I(a[15]), I(a[16]));
    if (fn == "mp_plan_add_expand_reduce")
        return mp_plan_add_expand_reduce(p, F(a[0]), F(a[1]), F(a[2]), F(a[3]), F(a[4]), F(a[5]), F(a[6]), F(a[7]), F(a[8]), F(a[9]), F(a[10]),
                                         F(a[11]), F(a[12]), F(a[13]), I(a[14]), I(a[15]), I(a[16]), I(a[17]), I(a[18]), I(a[19]));
    if (fn == "mp_plan_add_stem_conv")
        return mp_plan_add_stem_conv(p, F(a[0]), F(a[1]), F(a[2]), F(a[3]), I(a[4]), F(a[5]), I(a[6]), I(a[7]), I(a[8]));
    if (fn == "mp_plan_add_stem_conv_f16")
        return mp_plan_add_stem_conv_f16(p, F(a[0]), F(a[1]), F(a[2]), F(a[3]), I(a[4]), V(a[5]), I(a[6]), I(a[7]), I(a[8]));
    if (fn == "mp_plan_add_maxpool") return mp_plan_add_maxpool(p, F(a[0]), F(a[1]), I(a[2]), I(a[3]), I(a[4]), I(a[5]));
    if (fn == "mp_plan_add_fuse_sum")
        return mp_plan_add_fuse_sum(p, F(a[0]), F(a[1]), I(a[2]), F(a[3]), I(a[4]), F(a[5]), I(a[6]), F(a[7]), I(a[8]), I(a[9]), I(a[10]), I(a[11]),
                                    I(a[12]));
    if (fn == "mp_plan_add_fuse_sum_f16")
        return mp_plan_add_fuse_sum_f16(p, V(a[0]), V(a[1]), I(a[2]), V(a[3]), I(a[4]), V(a[5]), I(a[6]), V(a[7]), I(a[8]), I(a[9]), I(a[10]), I(a[11]),
                                        I(a[12]));
    if (fn == "mp_plan_add_layout_f16") return mp_plan_add_layout_f16(p, I(a[0]), V(a[1]), V(a[2]), I(a[3]), I(a[4]), I(a[5]), I(a[6]));
    if (fn == "mp_plan_add_concat")
        return mp_plan_add_concat(p, V(a[0]), I(a[1]), V(a[2]), I(a[3]), V(a[4]), I(a[5]), I(a[6]), I(a[7]), I(a[8]));
    if (fn == "mp_plan_add_col_slice") return mp_plan_add_col_slice(p, V(a[0]), V(a[1]), I(a[2]), I(a[3]), I(a[4]), I(a[5]), I(a[6]));
    fprintf(stderr, "unknown function %s\n", fn.c_str());
    return 1000;
}

int main(int argc, char** argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: %s tests/golden/plan_calls.txt\n", argv[0]);
        return 2;
    }
    std::ifstream in(argv[1]);
    if (!in) {
        fprintf(stderr, "cannot read %s\n", argv[1]);
        return 2;
    }
    mp_plan* plan = mp_plan_create();
    if (!plan) return 2;
    std::string line;
    int64_t info[12];
    long long checksum = 0;
    int n_calls = 0;
    while (std::getline(in, line)) {
        std::istringstream ls(line);
        std::string fn, tok;
        if (!(ls >> fn)) continue;
        std::vector<Arg> args;
        bool no_plan = false;
        while (ls >> tok) {
            Arg a;
            if (tok == "noplan") { no_plan = true; continue; }
            if (tok.rfind("d:", 0) == 0) {
                a.is_desc = true;
                int32_t f[20] = {};  // mp_conv_desc: twenty int32 fields, in declaration order
                static_assert(sizeof(mp_conv_desc) == sizeof(f), "mp_conv_desc is twenty int32 fields");
                std::istringstream ds(tok.substr(2));
                std::string v;
                for (int i = 0; i < 20 && std::getline(ds, v, ','); ++i) f[i] = (int32_t)std::stoll(v);
                memcpy(&a.d, f, sizeof(f));
            } else if (tok != "null") {
                a.v = std::stoll(tok);
            }
            args.push_back(a);
        }
        args.resize(24);  // (a short line reads nulls, not past the end)
        const int rc = call(fn, no_plan ? nullptr : plan, args);
        if (rc == 1000) return 2;
        const int size = mp_plan_size(plan);
        printf("%s rc %d size %d\n", fn.c_str(), rc, size);
        ++n_calls;
        for (int i = 0; i < size; ++i) {  // every entry, after every call: the vector has grown past several reallocations by the end
            if (mp_plan_entry_info(plan, i, info) != MP_OK) return 3;
            for (int j = 0; j < 12; ++j) checksum += info[j] * (j + 1);
        }
    }
    const int size = mp_plan_size(plan);
    for (int i = 0; i < size; ++i) {
        mp_plan_entry_info(plan, i, info);
        printf("entry %d:", i);
        for (int j = 0; j < 12; ++j) printf(" %lld", (long long)info[j]);
        printf("\n");
    }
    const int bad = (mp_plan_entry_info(plan, -1, info) != MP_ERR_SHAPE) + (mp_plan_entry_info(plan, size, info) != MP_ERR_SHAPE);
    mp_plan_destroy(plan);
    printf("%d calls, %d entries, info checksum %lld\n", n_calls, size, checksum);
    return bad ? 3 : 0;
}
