// The one text of the layer refusals (dxrexperiments_amd/csrc/rt_skeleton.h: rt_skeleton_layers_refusal; host code without HIP) as a CPU
// program of its own, for g++ -fsanitize=address,undefined (tests/test_skeleton_blend_abi.py).  For every code 1 .. 9 of
// rt_skeleton_validate_layers: a list of two layers for each of two actors whose bad entry is actor 1's layer 1 where the code allows it
// (4 and 9 are about layer 0; 1 and 2 name no layer), held to the validators, and the refusal in the skeleton's form (actor 1's list alone,
// under rt_skeleton_set_blend) and in the crowd's (both actors, under rt_crowd_set_blend) against WANT, message and error class.
// WANT was not typed: it is the output of the two nine-way switches this function replaced -- rt_skeleton_set_blend's in rt_skeleton.hip and
// check_layers' in rt_crowd.hip, as they stood in the commit before it, copied into a program in which rt_set_error prints -- run over
// list_for() below.  The lists live in heap blocks of exactly their size, so that a read past either end is a report.
//   layer_refusals_sanitized
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../dxrexperiments_amd/csrc/rt_crowd.h"

static const uint32_t N_ACTORS = 2, N_LAYERS = 2, N_CLIPS = 3, N_MASKS = 2;
// what rt_pose_source (rt_internal.h, which needs HIP) says of a skeleton and of a crowd; the Python test holds that header to these
static const char *const NOUN[2] = {"skeleton", "crowd"};
static const char *const HINT[2] = {"rt_skeleton_set_pose or rt_skeleton_set_time gives it one", "rt_crowd_set_poses or rt_crowd_set_times gives it one"};

// The call that code `what` answers: the list (null for 1; for 2 a block of one byte that nobody may read), its n_layers and whether there is a pose
static rt_skeleton_layer *list_for(int what, uint32_t *n_layers, bool *posed)
{
    *n_layers = what == 2 ? RT_SKELETON_MAX_LAYERS + 1u : N_LAYERS;
    *posed = what != 9;
    if (what == 1) return nullptr;
    if (what == 2) return (rt_skeleton_layer *)malloc(1);
    rt_skeleton_layer *l = (rt_skeleton_layer *)malloc(sizeof(rt_skeleton_layer) * N_ACTORS * N_LAYERS);
    if (!l) return nullptr;
    for (uint32_t a = 0; a < N_ACTORS; a++) {
        l[a * N_LAYERS + 0] = {0u, 0.5f, 1.0f, RT_SKELETON_NO_MASK, RT_LAYER_BLEND};
        l[a * N_LAYERS + 1] = {1u, 0.25f, 0.5f, 0u, RT_LAYER_BLEND};
    }
    rt_skeleton_layer *base = &l[1 * N_LAYERS + 0], *top = &l[1 * N_LAYERS + 1];
    if (what == 3) top->mode = 7u;
    if (what == 4) base->mode = RT_LAYER_ADDITIVE;
    if (what == 5) top->clip = RT_SKELETON_CURRENT_POSE;
    if (what == 6) top->time = NAN;
    if (what == 7) top->clip = 5u;
    if (what == 8) top->mask = 4u;
    if (what == 9) base->clip = RT_SKELETON_CURRENT_POSE;
    return l;
}

struct Want {
    int rc;
    const char *skeleton, *crowd;
};
static const Want WANT[10] = {
    {0, "", ""},
    {RT_ERR_INVALID_ARG,
     "rt_skeleton_set_blend: null argument",
     "rt_crowd_set_blend: null argument"},
    {RT_ERR_INVALID_ARG,
     "rt_skeleton_set_blend: 9 layers: 1 .. 8 are supported",
     "rt_crowd_set_blend: 9 layers: 1 .. 8 are supported"},
    {RT_ERR_INVALID_ARG,
     "rt_skeleton_set_blend: layer 1 has mode 7: RT_LAYER_BLEND (0) or RT_LAYER_ADDITIVE (1)",
     "rt_crowd_set_blend: actor 1: layer 1 has mode 7: RT_LAYER_BLEND (0) or RT_LAYER_ADDITIVE (1)"},
    {RT_ERR_INVALID_ARG,
     "rt_skeleton_set_blend: layer 0 is additive: the base layer is RT_LAYER_BLEND",
     "rt_crowd_set_blend: actor 1: layer 0 is additive: the base layer is RT_LAYER_BLEND"},
    {RT_ERR_INVALID_ARG,
     "rt_skeleton_set_blend: layer 1 names RT_SKELETON_CURRENT_POSE: only layer 0 may",
     "rt_crowd_set_blend: actor 1: layer 1 names RT_SKELETON_CURRENT_POSE: only layer 0 may"},
    {RT_ERR_INVALID_ARG,
     "rt_skeleton_set_blend: the time of layer 1 is NaN",
     "rt_crowd_set_blend: actor 1: the time of layer 1 is NaN"},
    {RT_ERR_STATE,
     "rt_skeleton_set_blend: layer 1 names clip 5: the skeleton has 3 (rt_skeleton_add_clip adds one)",
     "rt_crowd_set_blend: actor 1: layer 1 names clip 5: the skeleton has 3 (rt_skeleton_add_clip adds one)"},
    {RT_ERR_STATE,
     "rt_skeleton_set_blend: layer 1 names mask 4: the skeleton has 2 (rt_skeleton_add_mask adds one)",
     "rt_crowd_set_blend: actor 1: layer 1 names mask 4: the skeleton has 2 (rt_skeleton_add_mask adds one)"},
    {RT_ERR_STATE,
     "rt_skeleton_set_blend: layer 0 names RT_SKELETON_CURRENT_POSE: the skeleton has no pose yet (rt_skeleton_set_pose or rt_skeleton_set_time gives it one)",
     "rt_crowd_set_blend: actor 1: layer 0 names RT_SKELETON_CURRENT_POSE: the crowd has no pose yet (rt_crowd_set_poses or rt_crowd_set_times gives it one)"},
};

int main()
{
    size_t refusals = 0;
    for (int what = 1; what <= 9; what++) {
        uint32_t n_layers = 0, bad = 0xFFFFFFFFu, a = 0xFFFFFFFFu;
        bool posed = true;
        rt_skeleton_layer *layers = list_for(what, &n_layers, &posed);
        if (what != 1 && !layers) return 3;
        char msg[512], tiny[16];
        // the skeleton's form: actor 1's list
        const rt_skeleton_layer *mine = what > 2 ? layers + N_LAYERS : layers;
        if (rt_skeleton_validate_layers(n_layers, mine, N_CLIPS, N_MASKS, posed, &bad) != what) return 5;
        int rc = rt_skeleton_layers_refusal(what, "rt_skeleton_set_blend", nullptr, bad, what > 2 ? &mine[bad] : nullptr, n_layers, N_CLIPS, N_MASKS, NOUN[0], HINT[0], msg,
                                            sizeof msg);
        if (rc != WANT[what].rc || strcmp(msg, WANT[what].skeleton)) {
            fprintf(stderr, "code %d, skeleton: %d \"%s\"\n  wanted %d \"%s\"\n", what, rc, msg, WANT[what].rc, WANT[what].skeleton);
            return 4;
        }
        // the crowd's form: both actors
        if (rt_crowd_validate_layers(N_ACTORS, n_layers, layers, N_CLIPS, N_MASKS, posed, &a, &bad) != what) return 5;
        const rt_skeleton_layer *l = what > 2 ? &layers[(size_t)a * n_layers + bad] : nullptr;
        rc = rt_skeleton_layers_refusal(what, "rt_crowd_set_blend", &a, bad, l, n_layers, N_CLIPS, N_MASKS, NOUN[1], HINT[1], msg, sizeof msg);
        if (rc != WANT[what].rc || strcmp(msg, WANT[what].crowd)) {
            fprintf(stderr, "code %d, crowd: %d \"%s\"\n  wanted %d \"%s\"\n", what, rc, msg, WANT[what].rc, WANT[what].crowd);
            return 4;
        }
        // a buffer too small for the message holds its beginning, terminated, and the class is the same
        if (rt_skeleton_layers_refusal(what, "rt_crowd_set_blend", &a, bad, l, n_layers, N_CLIPS, N_MASKS, NOUN[1], HINT[1], tiny, sizeof tiny) != rc ||
            strlen(tiny) != sizeof tiny - 1u || strncmp(tiny, msg, sizeof tiny - 1u))
            return 6;
        free(layers);
        refusals += 2;
    }
    printf("%zu refusals, 0 sanitizer reports\n", refusals);
    return 0;
}
