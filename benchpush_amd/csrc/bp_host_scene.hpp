// Host halves of the three scenario loaders (bp_load_scenarios, bp_load_maze, bp_bd_load): everything they do before the first HIP call.
// Plain C++17 without a HIP include, so that a CPU compiler and its sanitizers see the code the library runs: bp_capi.hip calls these builders and
// then only allocates, uploads and launches; tools/host_sanitize/host_sanitize.cpp calls the same builders on case files.
//
// A builder takes the configuration struct and the entry point's arrays, fills a local result and returns nullptr, or the refusal message that
// bp_last_error reports (the convention of rrt_config_error).  It never touches a handle: a refused load leaves nothing behind.
#pragma once
#include <cstdint>
#include <vector>

#include "../../include/benchpush_amd.h"
#include "bp_host_bd.hpp"

namespace bpgeom {

typedef std::vector<std::vector<Shape>> Trials;   // [trial][body slot]

// ---- the per-trial bodies as SoA tables (step 1 of upload_trials) ------------------------------------------------------------------------------------
struct D4 { double x, y, z, w; };   // the bytes of a double4
struct TrialTables {
    std::vector<int> nb, nv, kind;
    std::vector<P2> lv, ln;
    std::vector<D4> mass, pose, prop;
};
// body slots per trial: the largest trial, rounded up to a multiple of 8
static int trials_nbcap(const Trials &trials)
{
    size_t maxnb = 1;
    for (const auto &b : trials) maxnb = std::max(maxnb, b.size());
    return (int)((maxnb + 7) / 8 * 8);
}
// The tables with nbcap slots per trial, exactly as they are uploaded, and the scenario hash of the state records' layout id continued over them.
static const char *pack_trials(const Trials &trials, int nbcap, TrialTables &tt, unsigned long long &scen_hash)
{
    const size_t T = trials.size(), TB = T * (size_t)nbcap;
    tt.nb.assign(T, 0); tt.nv.assign(TB, 0); tt.kind.assign(TB, 0);
    tt.lv.assign(TB * BP_MAXV, P2{0, 0}); tt.ln.assign(TB * BP_MAXV, P2{0, 0});
    tt.mass.assign(TB, D4{0, 0, 0, 0}); tt.pose.assign(TB, D4{0, 0, 0, 0}); tt.prop.assign(TB, D4{0, 0, 0, 0});
    for (size_t t = 0; t < T; t++) {
        tt.nb[t] = (int)trials[t].size();
        for (size_t b = 0; b < trials[t].size(); b++) {
            const Shape &s = trials[t][b];
            if ((int)s.verts.size() > BP_MAXV) return "hull exceeds BP_MAXV vertices";
            const size_t o = t * (size_t)nbcap + b;
            tt.nv[o] = (int)s.verts.size();
            for (size_t i = 0; i < s.verts.size(); i++) { tt.lv[o * BP_MAXV + i] = s.verts[i]; tt.ln[o * BP_MAXV + i] = s.normals[i]; }
            tt.mass[o] = D4{s.m_inv, s.i_inv, s.cog.x, s.cog.y};
            tt.pose[o] = D4{s.p.x, s.p.y, s.angle, 0.0};
            tt.prop[o] = D4{s.radius, s.e, s.u, 0.0};
            tt.kind[o] = s.kind;
        }
    }
    unsigned long long sh = scen_hash;
    sh = bp_fnv1a(tt.nb.data(), sizeof(int) * tt.nb.size(), sh); sh = bp_fnv1a(tt.nv.data(), sizeof(int) * tt.nv.size(), sh);
    sh = bp_fnv1a(tt.kind.data(), sizeof(int) * tt.kind.size(), sh);
    sh = bp_fnv1a(tt.lv.data(), sizeof(P2) * tt.lv.size(), sh); sh = bp_fnv1a(tt.ln.data(), sizeof(P2) * tt.ln.size(), sh);
    sh = bp_fnv1a(tt.mass.data(), sizeof(D4) * tt.mass.size(), sh); sh = bp_fnv1a(tt.pose.data(), sizeof(D4) * tt.pose.size(), sh);
    sh = bp_fnv1a(tt.prop.data(), sizeof(D4) * tt.prop.size(), sh);
    scen_hash = sh;
    return nullptr;
}

static void set_material(Shape &s, double radius, double e, double u, int kind) { s.radius = radius; s.e = e; s.u = u; s.kind = kind; }

// ---- ship-ice-v0 ------------------------------------------------------------------------------------------------------------------------------------
static const char *ship_ice_scene(const bp_config &cf, int T, int F, int V, const double *verts, const int32_t *counts, const double *centres,
                                  const double *starts, const int32_t *nfloes, Trials &trials)
{
    trials.assign(T, {});
    for (int t = 0; t < T; t++) {
        std::vector<Shape> &bodies = trials[t];
        Shape ship;
        build_ship(cf.ship_verts, cf.num_ship_verts, starts[3 * t], starts[3 * t + 1], starts[3 * t + 2], ship);
        set_material(ship, cf.poly_radius, cf.elasticity, cf.friction, kind_of(1, 0, BODY_KINEMATIC)); // ship_ice_env.py:214-215
        bodies.push_back(ship);
        if (nfloes[t] > F) return "nfloes > F";
        for (int f = 0; f < nfloes[t]; f++) {
            const size_t o = (size_t)t * F + f;
            const int n = counts[o];
            if (n < 3) continue;
            if (n > V) return "vertex count > V";
            Shape s;
            if (!build_floe(verts + o * V * 2, n, centres[o * 2], centres[o * 2 + 1], cf.density, cf.poly_radius, s)) continue;
            set_material(s, cf.poly_radius, cf.elasticity, cf.friction, kind_of(2, 0, BODY_DYNAMIC));  // ship_ice_env.py:211-212
            bodies.push_back(s);
        }
    }
    return nullptr;
}

// ---- maze-NAMO-v0 -----------------------------------------------------------------------------------------------------------------------------------
struct MazeScene {
    Trials trials;
    std::vector<unsigned char> wall;      // [grid_h][grid_w] wall raster
    std::vector<double> norm, raw;        // BFS goal map: normalised, and un-normalised (info['goal_dt'])
    std::vector<double> obs_map;          // the observer's packed copy: sign = wall, magnitude = normalised distance (a wall cell's is exactly 1.0, never a zero)
};
static const char *maze_scene(const bp_config &cf, int grid_h, int grid_w, int T, int nbox, const double *centres, int nwalls, const double *walls,
                              const double *start, MazeScene &sc)
{
    sc.trials.assign(T, {});
    for (int t = 0; t < T; t++) {
        std::vector<Shape> &bodies = sc.trials[t];
        // robot: one KINEMATIC body with the main outline (type 1) + the wheels (type 0); friction stays at pymunk's
        // default 0 (Robot.sim sets mass and elasticity only, robot.py:90-105)
        const double *st3 = start + 3 * (size_t)t;   // start pose of this layout (maze_NAMO_env.py:229-245)
        for (int k = 0; k <= cf.num_wheels; k++) {
            Shape s;
            if (k == 0) build_kinematic_part(cf.ship_verts, cf.num_ship_verts, st3[0], st3[1], st3[2], s);
            else build_kinematic_part(cf.wheel_verts[k - 1], 4, st3[0], st3[1], st3[2], s);
            set_material(s, cf.poly_radius, cf.elasticity, 0.0, kind_of(k == 0 ? 1 : 0, 1, BODY_KINEMATIC));
            bodies.push_back(s);
        }
        for (int b = 0; b < nbox; b++) {
            const double ox = centres[((size_t)t * nbox + b) * 2], oy = centres[((size_t)t * nbox + b) * 2 + 1], sz = cf.obstacle_size;
            const double raw[8] = {ox + sz, oy + sz, ox - sz, oy + sz, ox - sz, oy - sz, ox + sz, oy - sz}; // maze_NAMO_env.py:317-320
            Shape s;
            if (!build_floe(raw, 4, ox, oy, cf.density, cf.poly_radius, s)) continue;
            set_material(s, cf.poly_radius, cf.elasticity, cf.friction, kind_of(2, 0, BODY_DYNAMIC));
            bodies.push_back(s);
        }
        for (int w = 0; w < nwalls; w++) {
            Shape s;
            build_wall(walls[4 * w], walls[4 * w + 1], walls[4 * w + 2], walls[4 * w + 3], s);
            set_material(s, cf.wall_radius, 0.5, 0.5, kind_of(3, 0, BODY_STATIC));            // sim_utils.py:177-180
            bodies.push_back(s);
        }
    }
    // static maps: wall raster + BFS goal map
    maze_maps(walls, nwalls, cf.wall_radius, cf.map_w, cf.map_h, grid_h, grid_w, cf.goal_x, cf.goal_y, sc.wall, sc.norm, sc.raw);
    sc.obs_map.resize(sc.norm.size());
    for (size_t i = 0; i < sc.norm.size(); i++) sc.obs_map[i] = sc.wall[i] ? -sc.norm[i] : sc.norm[i];
    return nullptr;
}
// the maps' part of the scenario hash (before the trial tables')
static unsigned long long maze_scene_hash(const MazeScene &sc, unsigned long long h)
{
    h = bp_fnv1a(sc.wall.data(), sc.wall.size(), h);
    h = bp_fnv1a(sc.norm.data(), sizeof(double) * sc.norm.size(), h);
    return bp_fnv1a(sc.raw.data(), sizeof(double) * sc.raw.size(), h);
}

// ---- box-delivery-v0 / area-clearing-v0 ----------------------------------------------------------------------------------------------------------------
struct BdScene {
    Trials trials;                        // agent main shape, 4 wheels + bumper, the boxes, the static obstacles
    std::vector<int> map_of_trial;        // [T] index into maps
    std::vector<BdMaps> maps;             // one per distinct obstacle layout (exact equality of the world polygons)
    std::vector<P2> recept_poly, recept_n;// [layout][4] box-delivery: world vertices and normals of the receptacle of the layout's first trial
    std::vector<unsigned char> robot_chan;// [local_px][local_px] robot_state_channel * 255
};
// robot_state_channel (box_delivery_env.py:124-131) * 255
static std::vector<unsigned char> bd_robot_channel(int lp, double robot_radius, double ppm)
{
    std::vector<unsigned char> chan((size_t)lp * lp, 0);
    const int rpw = (int)(2 * robot_radius * ppm);
    const int start = (int)std::floor((double)lp / 2 - (double)rpw / 2);
    for (int i = start; i < start + rpw; i++)
        for (int j = start; j < start + rpw; j++) {
            if (i < 0 || j < 0 || i >= lp || j >= lp) continue;
            const double a = ((double)i + 0.5) - (double)lp / 2, b = ((double)j + 0.5) - (double)lp / 2;
            if (std::sqrt(a * a + b * b) < (double)rpw / 2) chan[(size_t)i * lp + j] = 255;
        }
    return chan;
}
static const char *bd_scene(const bp_bd_config &cf, int T, int nbox, const double *starts, const double *boxes, int ns, const double *sverts,
                            const int32_t *scount, const double *spose, const double *srad, const int32_t *stype, BdScene &sc)
{
    sc = BdScene();
    sc.trials.assign(T, {});
    sc.map_of_trial.assign(T, 0);
    std::vector<std::vector<std::vector<P2>>> map_keys; // obstacle polygons of each distinct layout
    for (int t = 0; t < T; t++) {
        std::vector<Shape> &bodies = sc.trials[t];
        const double sx = starts[3 * t], sy = starts[3 * t + 1], sh = starts[3 * t + 2];
        {   // create_agent (sim_utils.py:20-73): main shape radius 0 / friction 1, wheels + bumper radius 0.02 / friction 0
            Shape s;
            build_agent_main(cf.robot_verts, 4, sx, sy, sh, s);
            set_material(s, 0.0, 0.01, 1.0, kind_of(1, 1, BODY_KINEMATIC));
            bodies.push_back(s);
            for (int k = 0; k < 5; k++) {
                Shape w;
                build_kinematic_part(k < 4 ? cf.wheel_verts[k] : cf.bumper_verts, 4, sx, sy, sh, w);
                set_material(w, 0.02, 0.01, 0.0, kind_of(0, 1, BODY_KINEMATIC));
                bodies.push_back(w);
            }
        }
        for (int b = 0; b < nbox; b++) {
            const double *bx = boxes + ((size_t)t * nbox + b) * 3;
            Shape s;
            if (!build_box(bx[0], bx[1], bx[2], cf.box_half, cf.box_density, 0.02, s)) return "degenerate box";
            set_material(s, 0.02, 0.01, 1.0, kind_of(2, 0, BODY_DYNAMIC));
            bodies.push_back(s);
        }
        std::vector<std::vector<P2>> obstacles;
        Shape recept;
        int nrec = 0;
        for (int k = 0; k < ns; k++) {
            const size_t o = (size_t)t * ns + k;
            const int n = scount[o];
            if (n == 0) continue;   // padding: trials may hold different numbers of columns
            if (n < 3 || n > 4) return "static polygons have 3 or 4 vertices";
            Shape s;
            build_static_poly(sverts + o * 8, n, spose[o * 3], spose[o * 3 + 1], spose[o * 3 + 2], s);
            if (cf.task == 1) set_material(s, srad[o], 0.0, 0.99, 0);   // area_clearing.py:446-474: pymunk default elasticity, friction 0.99
            else set_material(s, srad[o], 0.01, 1.0, 0);
            if (stype[o] == 4) {
                if (s.verts.size() != 4) return "the receptacle must be a quadrilateral";
                recept = s; nrec++;
                continue;            // the receptacle never produces a collision response (handlers :216-229): not a physics slot
            }
            s.kind = kind_of(3, 0, BODY_STATIC);
            bodies.push_back(s);
            obstacles.push_back(world_verts(s));
        }
        if (cf.task == 0 && nrec != 1) return "exactly one receptacle polygon per trial is required";
        if (cf.task == 1 && nrec != 0) return "area-clearing has no receptacle polygon";
        int mi = -1;
        for (size_t m = 0; m < map_keys.size() && mi < 0; m++) {
            bool same = map_keys[m].size() == obstacles.size();
            for (size_t q = 0; same && q < obstacles.size(); q++) {
                same = map_keys[m][q].size() == obstacles[q].size();
                for (size_t v = 0; same && v < obstacles[q].size(); v++) same = map_keys[m][q][v].x == obstacles[q][v].x && map_keys[m][q][v].y == obstacles[q][v].y;
            }
            if (same) mi = (int)m;
        }
        if (mi < 0) {
            BdMaps M;
            AcGeom G;
            G.nbd = cf.num_boundary_verts; G.nob = cf.num_outer_verts; G.ngoal = cf.num_goal_points;
            G.bd = cf.boundary; G.ob = cf.outer_boundary; G.goals = cf.goal_points; G.scale_max = cf.distance_scale_max;
            if (!bd_build_maps(obstacles, cf.room_length, cf.room_width, cf.ppm, cf.local_px, cf.local_w, cf.robot_radius, cf.robot_half_width,
                               cf.recept_x, cf.recept_y, cf.sp_channel_scale, M, cf.task, &G, cf.task == 0 && cf.invert_receptacle_map != 0))
                return "free space does not fit the small-map window";
            sc.maps.push_back(M);
            map_keys.push_back(obstacles);
            mi = (int)map_keys.size() - 1;
            if (cf.task == 0) {   // t is the layout's first trial
                const std::vector<P2> wv = world_verts(recept);
                sc.recept_poly.insert(sc.recept_poly.end(), wv.begin(), wv.end());
                sc.recept_n.insert(sc.recept_n.end(), recept.normals.begin(), recept.normals.end());
            }
        }
        sc.map_of_trial[t] = mi;
    }
    sc.robot_chan = bd_robot_channel(cf.local_px, cf.robot_radius, cf.ppm);
    return nullptr;
}
// the maps' part of the scenario hash (after the trial tables')
static unsigned long long bd_scene_hash(const BdScene &sc, unsigned long long h)
{
    h = bp_fnv1a(sc.map_of_trial.data(), sizeof(int) * sc.map_of_trial.size(), h);
    for (size_t m = 0; m < sc.maps.size(); m++) {
        const BdMaps &M = sc.maps[m];
        h = bp_fnv1a(M.free_bits.data(), sizeof(unsigned) * M.free_bits.size(), h);
        h = bp_fnv1a(M.thin_bits.data(), sizeof(unsigned) * M.thin_bits.size(), h);
        h = bp_fnv1a(M.edt.data(), sizeof(unsigned short) * M.edt.size(), h);
        h = bp_fnv1a(M.recept.data(), sizeof(float) * M.recept.size(), h);
        h = bp_fnv1a(M.small_free.data(), M.small_free.size(), h);
        if (!sc.recept_poly.empty()) h = bp_fnv1a(&sc.recept_poly[4 * m], sizeof(P2) * 4, h);
    }
    return h;
}

} // namespace bpgeom
