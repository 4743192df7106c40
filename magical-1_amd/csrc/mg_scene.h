// mg_scene.h -- explicit scenes (include/magical_sim.h: mg_scene, mg_get_scene, mg_reset_scene): the layout of an env as
// data.  reset_env (mg_reset.h) decides the arguments of inst_goal / inst_block / inst_robot from the task's constants
// and the env's RNG; here they come from a caller's record.  Device side: the record's row load, its validation, the
// build (reset_env's prologue and epilogue around one inst_* call per entity), the overlap check and the read-back.
#pragma once
#include "../../include/magical_sim.h"
#include "mg_reset.h"

static_assert(sizeof(mg_scene_ent) == 56 && sizeof(mg_scene) == 792 && sizeof(mg_scene) % 8 == 0, "mg_scene layout");
static_assert(sizeof(((mg_scene *)0)->ent) / sizeof(mg_scene_ent) == MG_MAX_ENTS - 1, "mg_scene holds every entity slot");
#define MG_SCENE_WORDS ((int)(sizeof(mg_scene) / 8))   // 99 8-byte words: a row is 8-byte, not 16-byte, aligned

// what the handle allows: its task and flags, the slot caps of its scenes (step_caps) and whether the step kernel's
// constraint list is compiled (forms 5 / 6: the counts must then be the caps exactly)
struct SceneCfg { int task, flags; StepCaps caps; int exact; };

enum { MG_SCENE_OK = 0, MG_SCENE_UNSELECTED = -1, MG_SCENE_BAD_ORDER = 1, MG_SCENE_BAD_RANGE = 2, MG_SCENE_NO_FIT = 3,
       MG_SCENE_BAD_TARGET = 4 };
#define MG_SCENE_GOAL_MIN 0.1
#define MG_SCENE_GOAL_MAX 0.8   // RAND_GOAL_MAX_SIZE (randomise_hw's default mx, mg_reset.h:417): the render classes' caps
#define MG_SCENE_ANGLE_MAX 100.0

// Row e of the caller's array -> row[0 .. 99) in LDS (16-byte aligned), by one wavefront.  Rows are 792 bytes apart, so
// every other one starts on the odd half of a 16-byte line: the 49 aligned 16-byte loads cover words [head, head + 98)
// and the word left over, the first or the last, is one 8-byte load.  Nothing outside the row's own bytes is read.
MG_DEV void scene_load_row(const mg_scene *__restrict__ scenes, int e, uint64_t *row, int lane) {
    const char *src = (const char *)(scenes + e);
    const int head = (int)(((uintptr_t)src >> 3) & 1u);
    if (lane < (MG_SCENE_WORDS - 1) / 2) {
        const uint4 v = *(const uint4 *)(src + 8 * head + 16 * lane);
        row[head + 2 * lane] = (uint64_t)v.x | ((uint64_t)v.y << 32);
        row[head + 2 * lane + 1] = (uint64_t)v.z | ((uint64_t)v.w << 32);
    } else if (lane == (MG_SCENE_WORDS - 1) / 2) {
        const int w = head ? 0 : MG_SCENE_WORDS - 1;
        row[w] = *(const uint64_t *)(src + 8 * w);
    }
}

// The entity order of a task's scene with n entities after the arena (the add order of reset_env's branch for the task):
// ngoal goals, then nblk blocks, then the robot -- or the robot first (MoveToCorner, PickAndPlace).  ok: n is a count
// the task's scorer is defined for (the lower ends of the reference's count ranges; the upper end is the handle's caps).
struct SceneOrder { int ngoal, nblk, robot_first, ok; };
MG_DEV SceneOrder scene_order(int task, int n) {
    SceneOrder o = {0, 0, 0, 0};
    if (n < 1 || n > MG_MAX_ENTS - 1) return o;
    switch (task) {
    case MG_TASK_MOVE_TO_REGION: o.ngoal = 1; o.nblk = n - 2; o.ok = o.nblk == 0; break;
    case MG_TASK_MOVE_TO_CORNER: o.robot_first = 1; o.nblk = n - 1; o.ok = o.nblk == 1; break;
    case MG_TASK_CLUSTER_COLOUR:
    case MG_TASK_CLUSTER_SHAPE: o.nblk = n - 1; o.ok = o.nblk >= 7; break;
    case MG_TASK_MAKE_LINE: o.nblk = n - 1; o.ok = o.nblk >= 3; break;
    case MG_TASK_FIND_DUPE: o.ngoal = 1; o.nblk = n - 2; o.ok = o.nblk >= 3; break;   // outer blocks, then the query
    case MG_TASK_FIX_COLOUR: o.ngoal = o.nblk = (n - 1) / 2; o.ok = (n & 1) && o.nblk >= 2; break;
    case MG_TASK_PICK_AND_PLACE: o.robot_first = 1; o.nblk = n - 1; o.ok = o.nblk == 3; break;
    default: o.ngoal = 1; o.nblk = n - 2; o.ok = o.nblk >= 1; break;   // MatchRegions
    }
    return o;
}
MG_DEV int scene_kind_at(const SceneOrder &o, int n, int i) {
    if (o.robot_first) return i == 0 ? MG_ENT_ROBOT : MG_ENT_BLOCK;
    return i < o.ngoal ? MG_ENT_GOAL : i < n - 1 ? MG_ENT_BLOCK : MG_ENT_ROBOT;
}

MG_DEV bool scene_within(double v, double bound) { return fabs(v) <= bound; }   // false for NaN

// The record's status (MG_SCENE_*, the lowest code that applies).  It reads the record and the library only; every
// index the build forms from caller data (entity, body, shape and constraint slots, ent[target_ent], the block type's
// library row) is bounded by a test here.
MG_DEV int scene_status(const mg_scene &R, const mg_library *L, const SceneCfg &c) {
    const int n = R.n_ents;
    const SceneOrder o = scene_order(c.task, n);
    if (!o.ok) return MG_SCENE_BAD_ORDER;
    for (int i = 0; i < n; i++)
        if (R.ent[i].kind != scene_kind_at(o, n, i)) return MG_SCENE_BAD_ORDER;
    if (c.task == MG_TASK_MATCH_REGIONS) {
        bool any = false;
        for (int i = 1; i < n - 1; i++) any = any || R.ent[i].colour == R.ent[0].colour;
        if (!any) return MG_SCENE_BAD_ORDER;
    }
    bool bad = false;
    for (int i = 0; i < 5; i++) bad = bad || !(R.pv[i] > 0.0 && R.pv[i] <= DBL_MAX);
    for (int i = 0; i < n; i++) {
        const mg_scene_ent &t = R.ent[i];
        bad = bad || (t.flags & ~1) != 0 || !scene_within(t.x, 1.0) || !scene_within(t.y, 1.0);
        if (t.kind == MG_ENT_GOAL) {
            bad = bad || t.type != 0 || t.colour < MG_COL_RED || t.colour > MG_COL_YELLOW || !(t.angle == 0.0) ||
                  !(t.h >= MG_SCENE_GOAL_MIN && t.h <= MG_SCENE_GOAL_MAX) || !(t.w >= MG_SCENE_GOAL_MIN && t.w <= MG_SCENE_GOAL_MAX);
        } else {
            bad = bad || !scene_within(t.angle, MG_SCENE_ANGLE_MAX) || !(t.h == 0.0) || !(t.w == 0.0);
            if (t.kind == MG_ENT_BLOCK)
                bad = bad || t.type < 0 || t.type >= MG_NUM_SHAPE_TYPES || t.colour < MG_COL_RED || t.colour > MG_COL_YELLOW;
            else
                bad = bad || t.type != 0;   // the robot's colour is ignored
        }
    }
    if (c.task == MG_TASK_PICK_AND_PLACE) bad = bad || !scene_within(R.target_xy[0], 1.0) || !scene_within(R.target_xy[1], 1.0);
    if (bad) return MG_SCENE_BAD_RANGE;
    int nb = 6 + o.nblk, ns = 5, nc = 10 + 2 * o.nblk;   // add_robot: 6 bodies, 5 shapes, 10 constraints; add_block: 1, its shapes, 2
    for (int i = 0; i < n; i++)
        if (R.ent[i].kind == MG_ENT_BLOCK) ns += L->block_nshapes[R.ent[i].type];
    const bool fits = nb <= c.caps.nb && ns <= c.caps.ns && nc <= c.caps.nc && nb <= MG_MAX_BODIES && ns <= MG_MAX_SHAPES &&
                      nc <= MG_MAX_CONS;
    if (!fits || (c.exact && !(nb == c.caps.nb && ns == c.caps.ns && nc == c.caps.nc))) return MG_SCENE_NO_FIT;
    if (c.task == MG_TASK_PICK_AND_PLACE &&
        !(R.target_ent >= 0 && R.target_ent < n && R.ent[R.target_ent].kind == MG_ENT_BLOCK))
        return MG_SCENE_BAD_TARGET;
    return MG_SCENE_OK;
}

// The pose reset_env instantiates the task's robot at (its inst_robot calls, mg_reset.h:499, 539 with CC_ROBOT at :441,
// 561, 594, 643, 669, 736; false for MoveToCorner, whose pose is drawn, :508-509).  The eye bodies are instantiated at
// the origin whatever that pose is (add_robot, mg_reset.h:169) and the layout sampler's rigid shifts carry them along
// from there, so a robot at another pose has its eyes at pose + R(angle - a0) (0 - p0): scene_build puts them there --
// at the origin, exactly, for the task's own pose.  Nothing reads an eye's position (no shape; a rotary spring).
MG_DEV bool scene_robot_origin(int task, double &x, double &y, double &a) {
    switch (task) {
    case MG_TASK_MOVE_TO_REGION: x = 0.058; y = 0.53; a = -2.13; return true;
    case MG_TASK_CLUSTER_COLOUR: x = CC_ROBOT[0][0]; y = CC_ROBOT[0][1]; a = CC_ROBOT[0][2]; return true;
    case MG_TASK_CLUSTER_SHAPE: x = CC_ROBOT[1][0]; y = CC_ROBOT[1][1]; a = CC_ROBOT[1][2]; return true;
    case MG_TASK_MAKE_LINE: x = 0.702; y = -0.255; a = 0.347; return true;
    case MG_TASK_FIND_DUPE: x = -0.57; y = 0.25; a = 3.83; return true;
    case MG_TASK_FIX_COLOUR: x = 0.368; y = 0.586; a = 0.718; return true;
    case MG_TASK_PICK_AND_PLACE: x = 0.0; y = 0.0; a = 0.55 * 3.141592653589793; return true;
    case MG_TASK_MATCH_REGIONS: x = -0.5; y = 0.1; a = -3.141592653589793 * 1.2; return true;
    default: return false;
    }
}

// Env e <- the validated record R: what reset_env leaves for a variant without layout randomisation whose constants and
// draws are R's.  Called by every lane of the env's wavefront with the same values, as reset_env is in reset_kernel.
MG_DEV void scene_build(const MGState &S, const mg_library *L, int e, const mg_scene &R, const SceneCfg &c) {
    const size_t N = (size_t)S.N;
    const int n = R.n_ents;
    const SceneOrder o = scene_order(c.task, n);
    // reset_env's prologue (mg_reset.h:477-488) with pv from the record; the MT19937 rows are not touched
    S.episode_steps[e] = 0;
    S.overflow[e] &= ~2;
    for (int i = 0; i < MG_MAX_ARB; i++) { AT(S.akey, i) = -1; AT(S.acount, i) = 0; AT(S.astate, i) = ARB_FIRST; }
    S.nactive[e] = 0; S.stamp[e] = 0; S.curr_dt[e] = 0.0; S.nents[e] = 0; S.goal_ent[e] = -1;
    S.target_speed[e] = 0.0; S.rel_turn[e] = 0.0; S.target_finger[e] = 0.0;
    for (int i = 0; i < 5; i++) S.pv[i * N + e] = R.pv[i];
    Builder B = {0, 0, 0, 4}; // arena segments hold hashids 0..3
    new_entity(S, e, MG_ENT_ARENA, 0, MG_COL_GREY, 0, 0, 0, 0);
    int star_groups = 0;
    const mg_scene_ent &query = R.ent[n >= 2 ? n - 2 : 0];   // FindDupe's query block
    for (int i = 0; i < n; i++) {
        const mg_scene_ent &t = R.ent[i];
        const int ent = i + 1;
        if (t.kind == MG_ENT_GOAL) {
            inst_goal(S, e, B, t.x, t.y, t.h, t.w, t.colour);
            AT(S.ex, ent) = t.x; AT(S.ey, ent) = t.y;   // the centre as given (inst_goal derives it from a corner)
        } else if (t.kind == MG_ENT_ROBOT) {
            inst_robot(S, L, e, B, t.x, t.y, t.angle);
            double x0, y0, a0;
            if (scene_robot_origin(c.task, x0, y0, a0)) {
                const V2 r = rotated(v2(0.0 - x0, 0.0 - y0), t.angle - a0);
                const int eye0 = S.robot_body0[e] + 2;   // add_robot: body, control, two eyes, two fingers
                for (int k = 0; k < 2; k++) { AT(S.bpx, eye0 + k) = t.x + r.x; AT(S.bpy, eye0 + k) = t.y + r.y; }
            }
        } else {
            int role = 0;   // the rule the task's reset applies (mg_reset.h:589, 640, 729-733)
            if (c.task == MG_TASK_FIND_DUPE) role = (t.colour == query.colour && t.type == query.type) ? 1 : 2;
            else if (c.task == MG_TASK_FIX_COLOUR) role = t.colour == R.ent[i - o.nblk].colour ? 1 : 2;
            else if (c.task == MG_TASK_MATCH_REGIONS) role = t.colour == R.ent[0].colour ? 1 : 2;
            inst_block(S, L, e, B, t.type, t.colour, role, t.x, t.y, t.angle, star_groups);
        }
    }
    if (c.task == MG_TASK_PICK_AND_PLACE) {   // mg_reset.h:678-698
        const mg_scene_ent &t = R.ent[R.target_ent];
        int tid = 0, cid = 0;
        for (int k = 0; k < 4; k++) {
            if (MG_SHAPE_TYPES[k] == t.type) tid = k;
            if (MG_SHAPE_COLOURS[k] == t.colour) cid = k;
        }
        S.tgt_x[e] = R.target_xy[0]; S.tgt_y[e] = R.target_xy[1];
        S.tgt_ids[e] = tid; S.tgt_ids[N + e] = cid;
        S.tgt_ent[e] = R.target_ent + 1;
        if (S.target_out) {
            double *out = S.target_out + 4 * (size_t)e;
            out[0] = tid; out[1] = cid; out[2] = S.tgt_x[e]; out[3] = S.tgt_y[e];
        }
    }
    S.nbodies[e] = B.nb; S.nshapes[e] = B.ns; S.ncons[e] = B.nc;
    // reset_env's epilogue (mg_reset.h:748-751): disabled entities collide with nothing for the episode
    for (int i = 0; i < n; i++)
        if (R.ent[i].flags & 1) ent_set_enabled(S, e, i + 1, 0);
    for (int k = 0; k < B.ns; k++)
        if (!AT(S.scat, k)) AT(S.sgroup, k) = (int16_t)(AT(S.sgroup, k) | MG_GROUP_OFF);
}

// The entities ent's overlap query ignores, by the rule of the task's layout sampler (mg_reset.h:602-608: FindDupe's
// sensor, robot and outer blocks ignore the query block, which ignores the sensor; :651-661: FixColour's regions and
// robot ignore the blocks, and block i ignores region i)
MG_DEV uint32_t scene_ignore(const MGState &S, int e, int task, int ent) {
    const int nents = S.nents[e];
    if (task == MG_TASK_FIND_DUPE) {
        const int q = nents - 2;
        return ent == q ? 1u << 1 : 1u << q;
    }
    if (task == MG_TASK_FIX_COLOUR) {
        const int nr = (nents - 2) / 2;
        if (ent > nr && ent <= 2 * nr) return 1u << (ent - nr);
        uint32_t blocks = 0u;
        for (int i = 0; i < nr; i++) blocks |= 1u << (1 + nr + i);
        return blocks;
    }
    return 0u;
}

// the reset's own overlap test on env e as it stands, by the env's wavefront (query_hits splits each query's candidates
// over the lanes): does any enabled entity hit a wall, an enabled goal or a shape it does not ignore?
MG_DEV bool scene_overlaps(const MGState &S, const mg_library *L, int e, int task, int lane) {
    const int nents = S.nents[e];
    bool hit = false;
    for (int ent = 1; ent < nents && !hit; ent++)
        if (ent_enabled(S, e, ent)) hit = entity_collides(S, L, e, ent, scene_ignore(S, e, task, ent), lane);
    return hit;
}

// env e's current layout -> *o (every byte of the record is written)
MG_DEV void scene_read(const MGState &S, int e, int task, mg_scene *o) {
    const size_t N = (size_t)S.N;
    const int n = min(max(S.nents[e] - 1, 0), MG_MAX_ENTS - 1);   // (0 before the env's first reset)
    const bool pnp = task == MG_TASK_PICK_AND_PLACE;
    o->n_ents = n;
    o->target_ent = pnp ? S.tgt_ent[e] - 1 : -1;
    for (int i = 0; i < 5; i++) o->pv[i] = S.pv[i * N + e];
    o->target_xy[0] = pnp ? S.tgt_x[e] : 0.0; o->target_xy[1] = pnp ? S.tgt_y[e] : 0.0;
    for (int i = 0; i < MG_MAX_ENTS - 1; i++) {
        mg_scene_ent t = {0, 0, 0, 0, 0.0, 0.0, 0.0, 0.0, 0.0};
        if (i < n) {
            const int ent = i + 1;
            t.kind = AT(S.ekind, ent); t.type = AT(S.etype, ent); t.colour = AT(S.ecol, ent);
            t.flags = ent_enabled(S, e, ent) ? 0 : 1;
            if (t.kind == MG_ENT_GOAL) {
                t.x = AT(S.ex, ent); t.y = AT(S.ey, ent); t.h = AT(S.eh, ent); t.w = AT(S.ew, ent);
            } else {
                const int b = AT(S.ebody0, ent);
                t.x = AT(S.bpx, b); t.y = AT(S.bpy, b); t.angle = AT(S.ba, b);
            }
        }
        o->ent[i] = t;
    }
}
