// Host probe of csrc/mg_stepforms.h for tests/test_host.py::test_step_forms_header: built with the host compiler
// under -fsanitize=address,undefined, prints as JSON (a) the LDS view that carve_view carves for every LDS pair of
// the form table, beside mg_step_lds_bytes, and (b) the (form, envs per workgroup, reported caps) the selection
// functions give over tasks x flags x overrides x env counts.
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include "mg_stepforms.h"

alignas(16) static unsigned char lds[160 * 1024];

static void view(int form, int blk, bool first) {
    const StepCaps c = step_form_caps(form);
    const StepViewRows d = {c.nb, c.ns, c.nc, c.na, 1};
    MGState V = {};
    carve_view(V, lds, c, blk);
    printf("%s{\"form\":%d,\"blk\":%d,\"lds_bytes\":%zu,\"N\":%d,\"cons_cap\":%d,\"arb_cap\":%d,\"arrays\":[", first ? "" : ",",
           form, blk, mg_step_lds_bytes(c, blk), V.N, V.cons_cap, V.arb_cap);
    const char *sep = "";
#define ROW(f, T, mult, rows) \
    printf("%s[\"%s\",%td,%zu,%zu]", sep, #f, (unsigned char *)V.f - lds, sizeof(T), (size_t)(mult) * d.rows * blk), sep = ",";
    MG_STEP_VIEW(ROW)
#undef ROW
    printf("]}");
}

int main(int argc, char **argv) {
    const int star_shapes = argc > 1 ? atoi(argv[1]) : 6;   // mg_library::block_nshapes[MG_SHAPE_STAR]
    printf("{\"views\":[");
    bool first = true;
#define VIEW(F, B) if (F != 0) view(F, B, first), first = false;
    MG_STEP_FORMS(VIEW)
#undef VIEW
    printf("],\"pairs\":[");
    const char *sep = "";
#define PAIR(F, B) printf("%s[%d,%d]", sep, F, B), sep = ",";
    MG_STEP_FORMS(PAIR)
#undef PAIR
    // MG_STEP_VARIANT (-1: unset), MG_STEP_BLK, MG_STEP_BLK0 (0: unset): each alone, then the combinations in use
    static const int ov[][3] = {{-1, 0, 0}, {0, 0, 0}, {1, 0, 0}, {2, 0, 0}, {3, 0, 0}, {4, 0, 0}, {5, 0, 0}, {6, 0, 0},
                                {7, 0, 0}, {-1, 8, 0}, {-1, 16, 0}, {-1, 4, 0}, {-1, 0, 1}, {-1, 0, 8}, {-1, 0, 16},
                                {0, 0, 1}, {0, 0, 8}, {0, 0, 16}, {5, 8, 0}, {5, 16, 0}, {5, 4, 0}, {6, 8, 0},
                                {6, 16, 0}, {6, 4, 0}, {4, 8, 0}};
    static const int envs[] = {1, 70, 1365, 2048, 4095, 4096, 8192};
    printf("],\"select\":[");
    first = true;
    for (int task = 0; task <= MG_TASK_PICK_AND_PLACE; task++)
        for (int flags : {0, (int)MG_RAND_SHAPE_TYPE, (int)MG_RAND_SHAPE_COUNT, MG_RAND_SHAPE_TYPE | MG_RAND_SHAPE_COUNT})
            for (const auto &o : ov) {
                const StepCaps task_caps = step_caps(task, flags, star_shapes);
                const int form = step_pick_form(task_caps, o[0]);
                const StepCaps c = step_reported_caps(form, task_caps);
                printf("%s[%d,%d,%d,%d,%d,%d,%d,%d,%d,%d", first ? "" : ",\n", task, flags, o[0], o[1], o[2], form, c.nb,
                       c.ns, c.nc, c.na);
                for (int n : envs) printf(",%d", step_pick_blk(form, n, 256, o[1], o[2]));
                printf("]");
                first = false;
            }
    printf("]}\n");
    return 0;
}
