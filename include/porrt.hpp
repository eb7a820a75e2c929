// porrt.hpp -- C++ host mirror of the reference's operator interface for the accelerated path, header-only,
// on top of the C ABI (porrt_hip.h).  Names, argument meaning and error behaviour follow cambyse/po-rrt:
//   ContinuousSampler / DiscreteSampler   src/sample_space.rs:6-60
//   SquareGoal / ObservationGoal          src/common.rs:304-350, src/rrt.rs:325-341
//   MapShelfDomain / Map                  src/map_shelves_io.rs:65-148, src/map_io.rs:67-161 (open, add_zones); the drawing functions
//                                         resize / draw_tree / draw_full_graph / draw_policy / draw_path / draw_zones_observability / save
//                                         (map_shelves_io.rs:276-457, map_io.rs:303-479) on a device canvas
//   RRTNode / RRTTree / RRT::plan(_several)  src/rrt.rs:14-62, 84-100, 183-246
//   PTO::grow_graph + PTOGraph + Reachability  src/pto.rs:55-139, src/pto_graph.rs:171-207, src/pto_reachability.rs
// The reference is Rust; this image has no Rust toolchain, so the compiled host is C++ (INTEGRATION.md has the
// Rust binding).  Panics of the reference become std::runtime_error.
#pragma once
#include "porrt_hip.h"

#include <algorithm>
#include <array>
#include <cmath>
#include <cctype>
#include <cstdint>
#include <fstream>
#include <memory>
#include <optional>
#include <sstream>
#include <stdexcept>
#include <string>
#include <unordered_set>
#include <utility>
#include <vector>

namespace po_rrt {

using State = std::array<double, 2>;
using WorldMask = uint64_t;          // bit w <-> world w (BitVec in the reference)

struct ContinuousSampler {           // sample_space.rs:6-28 (the reference hard-codes seed 0)
    State low, up;
    uint64_t seed = 0;
    ContinuousSampler(State l, State u, uint64_t s = 0) : low(l), up(u), seed(s) {}
};
struct DiscreteSampler {             // sample_space.rs:39-55
    uint64_t seed = 0;
    explicit DiscreteSampler(uint64_t s = 0) : seed(s) {}
};

struct SquareGoal {                  // common.rs:304-333
    std::vector<std::pair<State, WorldMask>> goal_to_validity;
    double max_dist;
    SquareGoal(std::vector<std::pair<State, WorldMask>> g, double d) : goal_to_validity(std::move(g)), max_dist(d) {
        if (goal_to_validity.empty()) throw std::runtime_error("should have at least one element");
    }
};
struct ObservationGoal {             // rrt.rs:325-341
    uint32_t zone_id;
};

// 8-bit gray raster, row-major; P5 and P2 PGM (what the reference loads through the `image` crate)
struct Raster {
    uint32_t W = 0, H = 0;
    std::vector<uint8_t> px;
    static Raster open(const std::string &path) {
        std::ifstream f(path, std::ios::binary);
        if (!f) throw std::runtime_error("Impossible to open image: " + path);
        std::string magic;
        f >> magic;
        auto next_int = [&]() {
            for (;;) {
                int c = f.peek();
                if (c == '#') { std::string line; std::getline(f, line); }
                else if (isspace(c)) f.get();
                else break;
            }
            int v; f >> v; return v;
        };
        Raster r;
        r.W = next_int(); r.H = next_int();
        int maxv = next_int();
        (void)maxv;
        r.px.resize((size_t)r.W * r.H);
        if (magic == "P5") { f.get(); f.read((char *)r.px.data(), (std::streamsize)r.px.size()); }
        else if (magic == "P2") { for (auto &p : r.px) p = (uint8_t)next_int(); }
        else throw std::runtime_error("Wrong image format!");
        return r;
    }
};

struct GridDomain {                  // common part of MapShelfDomain / Map
    Raster img, zones;
    State low, up;
    double visibility_distance = 0.0;
    int domain;
    bool has_zones = false;
    GridDomain(Raster r, State l, State u, int d) : img(std::move(r)), low(l), up(u), domain(d) {}
    void add_zones(const std::string &path, double visibility) { zones = Raster::open(path); visibility_distance = visibility; has_zones = true; }

    // ---- drawing functions (map_shelves_io.rs:276-457, map_io.rs:303-479), on a device canvas (porrt_canvas_*): the pictures are bit for
    // bit the reference's.  Ours: the canvas is made at the first draw call (on draw_device), so resize must come before the drawing (it
    // throws afterwards; the reference would resize the drawn image), where every
    // driver of the reference has it (pto.rs:313-317: m.resize(5); m.draw_full_graph(&graph); m.draw_zones_observability();
    // m.draw_policy(&policy); m.save(path)).  A planner is passed where the reference passes the graph or tree it holds (&pto.graph,
    // &rrt.rrttree): its nodes stay on the device.  Planner: RRT for draw_tree; PTO or PRM for draw_full_graph.
    using Color = std::array<uint8_t, 3>;
    int draw_device = 0;
    void resize(uint32_t factor) {
        if (canvas_) throw std::runtime_error("resize: call it before the first draw call");
        if (!factor) throw std::runtime_error("resize: factor 0");
        draw_factor_ *= factor;                  // (Nearest at f1 then f2 is Nearest at f1 * f2; the reference rounds ppm at every call, so after
                                                 //  SEVERAL resize calls its ppm can differ from ppm * (f1 * f2) in the last bit: call it once, as the drivers do)
    }
    template <class Planner> void draw_tree(const Planner &rrt) { draw_check(porrt_canvas_draw_tree(canvas(), rrt.context().get())); }
    template <class Planner> void draw_full_graph(const Planner &planner) { draw_check(porrt_canvas_draw_full_graph(canvas(), planner.context().get())); }
    template <class Policy_> void draw_policy(const Policy_ &policy) {
        std::vector<double> xy;
        std::vector<int64_t> parent;
        for (const auto &n : policy.nodes) { xy.push_back(n.state[0]); xy.push_back(n.state[1]); parent.push_back(n.parent ? (int64_t)*n.parent : -1); }
        draw_check(porrt_canvas_draw_policy(canvas(), xy.data(), parent.data(), parent.size()));
    }
    void draw_path(const std::vector<State> &path, Color color) {
        std::vector<double> xy;
        for (const State &s : path) { xy.push_back(s[0]); xy.push_back(s[1]); }
        draw_check(porrt_canvas_draw_path(canvas(), xy.data(), path.size(), color.data()));
    }
    void draw_zones_observability() { draw_check(porrt_canvas_draw_zones_observability(canvas())); }
    void save(const std::string &path) { draw_check(porrt_canvas_save_png(canvas(), path.c_str())); }
    struct porrt_draw_info draw_info() { struct porrt_draw_info i; draw_check(porrt_canvas_get_info(canvas(), &i)); return i; }

private:
    uint32_t draw_factor_ = 1;
    std::shared_ptr<porrt_canvas> canvas_;
    void draw_check(int rc) const { if (rc < 0) throw std::runtime_error(porrt_canvas_last_error(canvas_.get())); }
    porrt_canvas *canvas() {
        if (!canvas_) {
            porrt_ctx *c = porrt_create(draw_device);
            if (!c) throw std::runtime_error("porrt_create failed: no usable HIP device (there is no CPU fallback)");
            porrt_canvas *cv = nullptr;
            if (porrt_set_grid(c, img.px.data(), img.W, img.H, low.data(), up.data(), domain) >= 0 &&
                (!has_zones || porrt_set_zones(c, zones.px.data(), visibility_distance) >= 0))
                cv = porrt_canvas_create(c, draw_factor_);
            const std::string msg = porrt_last_error(c);
            porrt_destroy(c);                      // (the canvas outlives the context it was made from)
            if (!cv) throw std::runtime_error(msg);
            canvas_ = std::shared_ptr<porrt_canvas>(cv, porrt_canvas_destroy);
        }
        return canvas_.get();
    }
};
// the reference's colour table (map_shelves_io.rs:25-48)
namespace colors {
using Color = GridDomain::Color;
constexpr Color BLACK{0, 0, 0}, WHITE{255, 255, 255}, RED{255, 0, 0}, LIME{0, 255, 0}, BLUE{0, 0, 255}, YELLOW{255, 255, 0}, CYAN{0, 255, 255},
    MAGENTA{255, 0, 255}, MAROON{128, 0, 0}, OLIVE{128, 128, 0}, GREEN{0, 128, 0}, PURPLE{128, 0, 128}, TEAL{0, 128, 128}, NAVY{0, 0, 128},
    GRAY1{30, 30, 30}, GRAY2{60, 60, 60}, GRAY3{90, 90, 90}, GRAY4{120, 120, 120}, GRAY5{150, 150, 150}, GRAY6{180, 180, 180},
    GRAY7{210, 210, 210}, GRAY8{240, 240, 240};
}
struct MapShelfDomain : GridDomain { // map_shelves_io.rs:80-114
    MapShelfDomain(Raster r, State l, State u) : GridDomain(std::move(r), l, u, PORRT_DOMAIN_SHELF) {}
    static MapShelfDomain open(const std::string &path, State l, State u) { return MapShelfDomain(Raster::open(path), l, u); }
};
struct Map : GridDomain {            // map_io.rs:82-128
    Map(Raster r, State l, State u) : GridDomain(std::move(r), l, u, PORRT_DOMAIN_DOOR) {}
    static Map open(const std::string &path, State l, State u) { return Map(Raster::open(path), l, u); }
};

struct RRTNode {                     // rrt.rs:14-18
    State state;
    std::optional<size_t> parent_id;
    double dist_from_root;
};
struct RRTTree {                     // rrt.rs:20-62
    std::vector<RRTNode> nodes;
    std::vector<State> get_path_to(size_t id) const {
        std::vector<State> path;
        const RRTNode *n = &nodes[id];
        path.push_back(n->state);
        while (n->parent_id) { n = &nodes[*n->parent_id]; path.push_back(n->state); }
        return std::vector<State>(path.rbegin(), path.rend());
    }
};

class Context {
public:
    explicit Context(int device = 0) : c_(porrt_create(device)) {
        if (!c_) throw std::runtime_error("porrt_create failed: no usable HIP device (there is no CPU fallback)");
    }
    ~Context() { porrt_destroy(c_); }
    Context(const Context &) = delete;
    Context &operator=(const Context &) = delete;
    porrt_ctx *get() const { return c_; }
    int check(int rc) const { if (rc < 0) throw std::runtime_error(porrt_last_error(c_)); return rc; }
    void set_domain(const GridDomain &m) {
        check(porrt_set_grid(c_, m.img.px.data(), m.img.W, m.img.H, m.low.data(), m.up.data(), m.domain));
        if (m.has_zones) check(porrt_set_zones(c_, m.zones.px.data(), m.visibility_distance));
    }
    void set_goal(const SquareGoal &g) {
        std::vector<double> c;
        std::vector<uint64_t> m;
        for (auto &p : g.goal_to_validity) { c.push_back(p.first[0]); c.push_back(p.first[1]); m.push_back(p.second); }
        check(porrt_set_square_goal(c_, c.data(), m.data(), (uint32_t)m.size(), g.max_dist));
    }
    void set_goal(const ObservationGoal &g) { check(porrt_set_observation_goal(c_, g.zone_id)); }
private:
    porrt_ctx *c_;
};

// rrt.rs:78-246.  `fns` is the grid-backed validator (the Funcs adapter of map_shelves_tamp_rrt.rs:35-47);
// nullptr = the default RTTFuncs (everything valid, rrt.rs:64-76).
class RRT {
public:
    const Context &context() const { return ctx_; }          // (the drawing functions of MapShelfDomain / Map read the graph on its device)
    uint32_t batch_K = 1024;         // samples per GPU step; 1 = the reference's sequential loop
    RRT(const ContinuousSampler &s, const MapShelfDomain *fns, int device = 0) : ctx_(device) {
        if (fns) ctx_.set_domain(*fns);
        ctx_.check(porrt_set_sampler(ctx_.get(), s.low.data(), s.up.data(), s.seed));
    }
    using Solution = std::pair<std::vector<State>, double>;
    template <class Goal>
    std::pair<std::optional<Solution>, RRTTree> plan(State start, const Goal &goal, double max_step, double search_radius,
                                                      size_t n_iter_min, size_t n_iter_max) {                     // rrt.rs:88-93
        auto [tree, finals] = grow_tree(start, goal, max_step, search_radius, n_iter_min, n_iter_max);
        return {get_best_solution(tree, finals), std::move(tree)};
    }
    template <class Goal>
    std::pair<std::vector<Solution>, RRTTree> plan_several(State start, const Goal &goal, double max_step, double search_radius,
                                                            size_t n_iter_min, size_t n_iter_max) {               // rrt.rs:95-100
        auto [tree, finals] = grow_tree(start, goal, max_step, search_radius, n_iter_min, n_iter_max);
        std::vector<Solution> out;
        for (size_t id : get_firstly_final_node_ids(tree, finals)) { auto p = tree.get_path_to(id); double c = path_cost(p); out.push_back({std::move(p), c}); }
        return {std::move(out), std::move(tree)};
    }
    // RRT::get_solutions (rrt.rs:195-221) of the last plan / plan_several / plan_batch, walked on the device (porrt_solutions: no
    // tree is downloaded): the firstly final nodes in ASCENDING NODE ID (the reference's order is a HashSet's), each with its path
    // from the root and the path's cost.  plan_several above keeps its host walk over the downloaded tree.
    std::vector<Solution> solutions() {
        porrt_ctx *c = ctx_.get();
        uint64_t ns = 0, nst = 0;
        ctx_.check(porrt_solutions(&c, 1, &ns, &nst, nullptr, nullptr, nullptr, 0, nullptr, 0));
        std::vector<uint64_t> ids(ns), lens(ns);
        std::vector<double> costs(ns), xy(2 * nst);
        if (ns) ctx_.check(porrt_solutions(&c, 1, &ns, &nst, ids.data(), lens.data(), costs.data(), ns, xy.data(), nst));
        std::vector<Solution> out;
        size_t at = 0;
        for (size_t s = 0; s < ns; ++s) {
            std::vector<State> p(lens[s]);
            for (size_t k = 0; k < lens[s]; ++k, ++at) p[k] = {xy[2 * at], xy[2 * at + 1]};
            out.push_back({std::move(p), costs[s]});
        }
        return out;
    }
    // Many independent queries at once (the TAMP layer's pattern, map_shelves_tamp_rrt.rs:163-291): every planner keeps
    // its own map, sampler state and result; all of them advance in one launch sequence (porrt_grow_batch), each running the
    // loop of rrt.rs:109 with the caller's n_iter_min / n_iter_max (the TAMP search passes 2500 / 10000, main.rs:532).  Same
    // results as calling plan() on each, several times the throughput.
    template <class Goal>
    static std::vector<std::pair<std::optional<Solution>, RRTTree>> plan_batch(const std::vector<RRT *> &planners, const std::vector<State> &starts,
                                                                                const Goal &goal, double max_step, double search_radius, size_t n_iter_min,
                                                                                size_t n_iter_max = 0) {
        if (n_iter_max < n_iter_min) n_iter_max = n_iter_min;
        std::vector<porrt_ctx *> cs;
        std::vector<double> st;
        for (size_t q = 0; q < planners.size(); ++q) {
            planners[q]->ctx_.set_goal(goal);
            cs.push_back(planners[q]->ctx_.get());
            st.push_back(starts[q][0]); st.push_back(starts[q][1]);
        }
        planners.at(0)->ctx_.check(porrt_grow_batch(cs.data(), (uint32_t)cs.size(), st.data(), max_step, search_radius, n_iter_min, n_iter_max, planners[0]->batch_K,
                                                    PORRT_MODE_RRT));
        std::vector<std::pair<std::optional<Solution>, RRTTree>> out;
        for (RRT *p : planners) {
            auto [tree, finals] = p->read_tree();
            out.push_back({get_best_solution(tree, finals), std::move(tree)});
        }
        return out;
    }
    // Cost of each planner's best path (get_best_solution, rrt.rs:183-193) evaluated on the device without fetching the
    // trees; +inf = "No solution found".  After plan_batch / a grow of all planners it is one kernel launch.
    static std::vector<double> best_costs(const std::vector<RRT *> &planners) {
        std::vector<porrt_ctx *> cs;
        for (RRT *p : planners) cs.push_back(p->ctx_.get());
        std::vector<double> costs(cs.size());
        planners.at(0)->ctx_.check(porrt_best_cost_batch(cs.data(), (uint32_t)cs.size(), costs.data()));
        return costs;
    }
private:
    Context ctx_;
    template <class Goal>
    std::pair<RRTTree, std::vector<size_t>> grow_tree(State start, const Goal &goal, double max_step, double search_radius,
                                                      size_t n_iter_min, size_t n_iter_max) {                     // rrt.rs:102-174
        ctx_.set_goal(goal);
        ctx_.check(porrt_grow(ctx_.get(), start.data(), max_step, search_radius, n_iter_min, n_iter_max, batch_K, PORRT_MODE_RRT));
        return read_tree();
    }
    std::pair<RRTTree, std::vector<size_t>> read_tree() {
        const size_t n = porrt_num_nodes(ctx_.get());
        std::vector<double> xy(2 * n), dist(n);
        std::vector<int64_t> parent(n);
        ctx_.check(porrt_get_tree(ctx_.get(), xy.data(), parent.data(), dist.data()));
        RRTTree t;
        t.nodes.resize(n);
        for (size_t j = 0; j < n; ++j) {
            t.nodes[j].state = {xy[2 * j], xy[2 * j + 1]};
            if (parent[j] >= 0) t.nodes[j].parent_id = (size_t)parent[j];
            t.nodes[j].dist_from_root = dist[j];
        }
        std::vector<uint64_t> f(porrt_num_final(ctx_.get()));
        if (!f.empty()) ctx_.check(porrt_get_final_ids(ctx_.get(), f.data()));
        return {std::move(t), std::vector<size_t>(f.begin(), f.end())};
    }
    static double norm2(const State &a, const State &b) { double dx = b[0] - a[0], dy = b[1] - a[1]; return std::sqrt(dx * dx + dy * dy); }
    static double path_cost(const std::vector<State> &p) { double s = 0; for (size_t i = 0; i + 1 < p.size(); ++i) s += norm2(p[i], p[i + 1]); return s; }
    static std::optional<Solution> get_best_solution(const RRTTree &t, const std::vector<size_t> &finals) {      // rrt.rs:183-193
        std::optional<Solution> best;
        for (size_t id : finals) { auto p = t.get_path_to(id); double c = path_cost(p); if (!best || c < best->second) best = Solution{std::move(p), c}; }
        return best;                   // nullopt <=> Err("No solution found")
    }
    static std::vector<size_t> get_firstly_final_node_ids(const RRTTree &t, const std::vector<size_t> &finals) { // rrt.rs:229-246
        std::unordered_set<size_t> fin(finals.begin(), finals.end()), first;
        for (size_t id : finals) {
            size_t cur = id;
            while (t.nodes[cur].parent_id && fin.count(*t.nodes[cur].parent_id)) cur = *t.nodes[cur].parent_id;
            first.insert(cur);
        }
        return std::vector<size_t>(first.begin(), first.end());
    }
};

// pto_graph.rs:171-207
struct PTOEdge { size_t id; size_t validity_id; };
struct PTONode { State state; size_t validity_id; std::vector<PTOEdge> parents, children; };
struct PTOGraph {
    std::vector<PTONode> nodes;
    std::vector<WorldMask> validities;
    void add_edge(size_t from, size_t to, size_t v) { nodes[from].children.push_back({to, v}); nodes[to].parents.push_back({from, v}); }
};

// pto.rs:15-149 (growth part) with the Reachability read-outs of pto_reachability.rs:54-90
using BeliefState = std::vector<double>;                       // common.rs: one probability per world

// common.rs:256-264
inline bool is_compatible(const BeliefState &belief_state, WorldMask validity) {
    for (size_t w = 0; w < belief_state.size(); ++w)
        if (belief_state[w] > 0.0 && !((validity >> w) & 1)) return false;
    return true;
}

enum class BeliefNodeType : uint8_t { Unknown = 0, Action = 1, Observation = 2 };     // belief_graph.rs:13-17

// BeliefGraph (belief_graph.rs:19-71) in CSR form: node i has node_type(i), children(i), parents(i); its graph node is
// i / n_beliefs, its belief reachable_belief_states[i % n_beliefs].
struct BeliefGraph {
    std::vector<BeliefState> reachable_belief_states;
    std::vector<uint8_t> node_types;
    std::vector<uint64_t> children_offsets, parents_offsets;
    std::vector<uint32_t> children_ids, parents_ids;
    size_t n_nodes() const { return node_types.size(); }
    size_t n_beliefs() const { return reachable_belief_states.size(); }
    BeliefNodeType node_type(size_t i) const { return (BeliefNodeType)node_types[i]; }
    size_t belief_id(size_t i) const { return i % n_beliefs(); }
    std::pair<const uint32_t *, const uint32_t *> children(size_t i) const { return {children_ids.data() + children_offsets[i], children_ids.data() + children_offsets[i + 1]}; }
    std::pair<const uint32_t *, const uint32_t *> parents(size_t i) const { return {parents_ids.data() + parents_offsets[i], parents_ids.data() + parents_offsets[i + 1]}; }
};

// common.rs:24-40
struct PolicyNode {
    State state;
    BeliefState belief_state;
    std::optional<size_t> parent;
    std::vector<size_t> children;
    size_t original_node_id = 0;
};
struct Policy {
    std::vector<PolicyNode> nodes;
    std::vector<size_t> leafs;
    double expected_costs = 0.0;
    const PolicyNode &leaf(size_t id) const { return nodes[leafs[id]]; }                             // common.rs:66-68
    std::vector<State> path_to_leaf(size_t id) const {                                               // common.rs:70-83
        std::vector<State> path;
        const PolicyNode *n = &leaf(id);
        path.push_back(n->state);
        while (n->parent) { n = &nodes[*n->parent]; path.push_back(n->state); }
        return std::vector<State>(path.rbegin(), path.rend());
    }
};

// pto_policy_refiner.rs:18-21
struct RefinmentStrategy {
    enum Kind { kReparent, kPartialShortCut } kind;
    double radius;
    size_t n_iterations;
    static RefinmentStrategy Reparent(double radius) { return {kReparent, radius, 0}; }
    static RefinmentStrategy PartialShortCut(size_t n_iterations) { return {kPartialShortCut, 0.0, n_iterations}; }
};

class PTO {
public:
    const Context &context() const { return ctx_; }          // (the drawing functions of MapShelfDomain / Map read the graph on its device)
    uint32_t batch_K = 256;
    PTOGraph graph;
    size_t n_it = 0;
    PTO(const ContinuousSampler &cs, const DiscreteSampler &ds, const GridDomain &fns, int device = 0) : ctx_(device) {
        ctx_.set_domain(fns);
        ctx_.check(porrt_set_sampler(ctx_.get(), cs.low.data(), cs.up.data(), cs.seed));
        ctx_.check(porrt_set_discrete_seed(ctx_.get(), ds.seed));
    }
    // Ok <=> returns true; false <=> Err("final nodes are not reached for each world") (pto.rs:134-138)
    bool grow_graph(State start, const SquareGoal &goal, double max_step, double search_radius, size_t n_iter_min, size_t n_iter_max) {
        ctx_.set_goal(goal);
        int rc = ctx_.check(porrt_grow(ctx_.get(), start.data(), max_step, search_radius, n_iter_min, n_iter_max, batch_K, PORRT_MODE_PTO));
        const size_t n = porrt_num_nodes(ctx_.get());
        n_it = porrt_num_iterations(ctx_.get());
        std::vector<double> xy(2 * n);
        std::vector<uint32_t> vid(n);
        ctx_.check(porrt_get_tree(ctx_.get(), xy.data(), nullptr, nullptr));
        ctx_.check(porrt_get_node_validity(ctx_.get(), vid.data()));
        reach_.assign(n, 0);
        ctx_.check(porrt_get_reach(ctx_.get(), reach_.data()));
        uint64_t val[65];
        int nv = porrt_get_validities(ctx_.get(), val);
        graph.validities.assign(val, val + nv);
        graph.nodes.assign(n, PTONode{});
        for (size_t j = 0; j < n; ++j) { graph.nodes[j].state = {xy[2 * j], xy[2 * j + 1]}; graph.nodes[j].validity_id = vid[j]; }
        const size_t E = porrt_num_edges(ctx_.get());
        std::vector<uint32_t> f(E), t(E), v(E);
        if (E) ctx_.check(porrt_get_edges(ctx_.get(), f.data(), t.data(), v.data()));
        for (size_t e0 = 0; e0 < E;) {             // per new node: neighbour->new edges, then new->neighbour (pto.rs:111-120)
            size_t e1 = e0;
            while (e1 < E && t[e1] == t[e0]) ++e1;
            for (size_t e = e0; e < e1; ++e) graph.add_edge(f[e], t[e], v[e]);
            for (size_t e = e0; e < e1; ++e) graph.add_edge(t[e], f[e], v[e]);
            e0 = e1;
        }
        final_ids_.assign(porrt_num_final(ctx_.get()), 0);
        final_masks_.assign(final_ids_.size(), 0);
        if (!final_ids_.empty()) { ctx_.check(porrt_get_final_ids(ctx_.get(), final_ids_.data())); ctx_.check(porrt_get_final_masks(ctx_.get(), final_masks_.data())); }
        return rc == PORRT_OK;
    }
    WorldMask reachability(size_t id) const { return reach_[id]; }                                   // pto_reachability.rs:54-56
    std::vector<size_t> get_final_nodes_for_world(size_t world) const {                              // pto_reachability.rs:58-63
        std::vector<size_t> out;
        for (size_t k = 0; k < final_ids_.size(); ++k)
            if (((reach_[final_ids_[k]] >> world) & 1) && ((final_masks_[k] >> world) & 1)) out.push_back((size_t)final_ids_[k]);
        return out;
    }
    int n_worlds() const { return porrt_n_worlds(ctx_.get()); }

    // PTO::build_belief_graph (pto.rs:185-259) on the graph of the last grow_graph.  belief_graph.nodes[i] is the belief
    // node of graph node i / n_beliefs and belief i % n_beliefs (the add_node order of pto.rs:198-201); children and
    // parents are views into the two id arrays, in the reference's Vec::push order.
    void build_belief_graph(const BeliefState &start_belief_state) {
        ctx_.check(porrt_build_belief_graph(ctx_.get(), start_belief_state.data(), (uint32_t)start_belief_state.size()));
        BeliefGraph &g = belief_graph;
        const size_t nb = porrt_bg_num_beliefs(ctx_.get()), nn = porrt_bg_num_nodes(ctx_.get()), ne = porrt_bg_num_edges(ctx_.get());
        const size_t nw = (size_t)n_worlds();
        std::vector<double> flat(nb * nw);
        ctx_.check(porrt_bg_get_beliefs(ctx_.get(), flat.data()));
        g.reachable_belief_states.assign(nb, BeliefState(nw));
        for (size_t b = 0; b < nb; ++b) g.reachable_belief_states[b].assign(flat.begin() + b * nw, flat.begin() + (b + 1) * nw);
        g.node_types.assign(nn, 0);
        g.children_offsets.assign(nn + 1, 0); g.parents_offsets.assign(nn + 1, 0);
        g.children_ids.assign(ne, 0); g.parents_ids.assign(ne, 0);
        ctx_.check(porrt_bg_get_node_types(ctx_.get(), g.node_types.data()));
        ctx_.check(porrt_bg_get_children(ctx_.get(), g.children_offsets.data(), g.children_ids.data()));
        ctx_.check(porrt_bg_get_parents(ctx_.get(), g.parents_offsets.data(), g.parents_ids.data()));
        // node_to_belief_nodes (pto.rs:196-208): Some(id) iff the belief is compatible with the node's validity
        node_to_belief_nodes.assign(graph.nodes.size(), std::vector<std::optional<size_t>>(nb));
        for (size_t n = 0; n < graph.nodes.size(); ++n)
            for (size_t b = 0; b < nb; ++b)
                if (is_compatible(g.reachable_belief_states[b], graph.validities[graph.nodes[n].validity_id])) node_to_belief_nodes[n][b] = n * nb + b;
    }
    BeliefGraph belief_graph;
    std::vector<std::vector<std::optional<size_t>>> node_to_belief_nodes;

    // pto.rs:261-275 (conditional_dijkstra, belief_graph.rs:89-175); the costs stay on the device, fetch = copy them out
    void compute_expected_costs_to_goals(bool fetch = true) {
        ctx_.check(porrt_bg_compute_expected_costs(ctx_.get()));
        if (fetch) {
            expected_costs_to_goals.assign(porrt_bg_num_nodes(ctx_.get()), 0.0);
            ctx_.check(porrt_bg_get_expected_costs(ctx_.get(), expected_costs_to_goals.data()));
        }
    }
    std::vector<double> expected_costs_to_goals;
    // pto.rs:277-283 (extract_policy, belief_graph.rs:177-263)
    Policy extract_policy() {
        Policy policy;
        const int64_t n = porrt_bg_extract_policy(ctx_.get(), nullptr, nullptr, nullptr, 0, &policy.expected_costs);
        if (n < 0) ctx_.check((int)n);
        std::vector<uint64_t> oid((size_t)n);
        std::vector<int64_t> par((size_t)n);
        std::vector<uint8_t> leaf((size_t)n);
        porrt_bg_extract_policy(ctx_.get(), oid.data(), par.data(), leaf.data(), (uint64_t)n, nullptr);
        const size_t nb = porrt_bg_num_beliefs(ctx_.get());
        std::vector<double> flat(nb * (size_t)n_worlds());
        ctx_.check(porrt_bg_get_beliefs(ctx_.get(), flat.data()));
        for (size_t k = 0; k < (size_t)n; ++k) {
            PolicyNode pn;
            pn.state = graph.nodes[oid[k] / nb].state;
            pn.belief_state.assign(flat.begin() + (oid[k] % nb) * n_worlds(), flat.begin() + (oid[k] % nb + 1) * n_worlds());
            pn.original_node_id = (size_t)oid[k];
            if (par[k] >= 0) { pn.parent = (size_t)par[k]; policy.nodes[(size_t)par[k]].children.push_back(k); }
            policy.nodes.push_back(std::move(pn));
            if (leaf[k]) policy.leafs.push_back(k);
        }
        return policy;
    }
    // extract_policy (belief_graph.rs:184-267) started at every belief node of starts, walked on the device in one call
    // (porrt_bg_extract_policies): one Policy per start, nullopt where there is none (statuses, when asked for: 1 no finite cost,
    // 2 the walk returns onto its own path, 3 an assertion of the reference fails, 4 more than option "policy_max_nodes" nodes)
    std::vector<std::optional<Policy>> extract_policies(const std::vector<size_t> &starts, std::vector<uint8_t> *statuses = nullptr) {
        const size_t nq = starts.size();
        std::vector<uint64_t> st(starts.begin(), starts.end()), off(nq + 1, 0);
        std::vector<uint8_t> status(nq + 1, 0);
        std::vector<double> cost(nq + 1, 0.0);
        const int64_t n = porrt_bg_extract_policies(ctx_.get(), st.data(), nq, off.data(), status.data(), cost.data(), nullptr, nullptr, nullptr, 0);
        if (n < 0) ctx_.check((int)n);
        n_policies_ = nq;
        std::vector<uint64_t> oid((size_t)n);
        std::vector<int64_t> par((size_t)n);
        std::vector<uint8_t> leaf((size_t)n);
        if (n > 0 && porrt_bg_get_policies(ctx_.get(), oid.data(), par.data(), leaf.data(), (uint64_t)n) != n) ctx_.check(PORRT_ERR_INVALID);
        const size_t nb = porrt_bg_num_beliefs(ctx_.get()), nw = (size_t)n_worlds();
        std::vector<double> flat(nb * nw);
        ctx_.check(porrt_bg_get_beliefs(ctx_.get(), flat.data()));
        std::vector<std::optional<Policy>> out(nq);
        for (size_t q = 0; q < nq; ++q) {
            if (status[q]) continue;
            Policy policy;
            policy.expected_costs = cost[q];
            for (size_t k = 0, o = (size_t)off[q]; o < (size_t)off[q + 1]; ++k, ++o) {
                PolicyNode pn;
                pn.state = graph.nodes[oid[o] / nb].state;
                pn.belief_state.assign(flat.begin() + (oid[o] % nb) * nw, flat.begin() + (oid[o] % nb + 1) * nw);
                pn.original_node_id = (size_t)oid[o];
                if (par[o] >= 0) { pn.parent = (size_t)par[o]; policy.nodes[(size_t)par[o]].children.push_back(k); }
                policy.nodes.push_back(std::move(pn));
                if (leaf[o]) policy.leafs.push_back(k);
            }
            out[q] = std::move(policy);
        }
        if (statuses) statuses->assign(status.begin(), status.begin() + nq);
        return out;
    }
    // PTOPolicyRefiner::new(&policy, ..).refine_solution(RefinmentStrategy::PartialShortCut(n_iterations)) (pto_policy_refiner.rs:87-124)
    // of the policy extract_policy() returned last: node states are the refined ones; a piece start the reference's recompose leaves
    // unconnected (after a one-node piece that branches) has no parent
    Policy refine_policy(size_t n_iterations) { return refine_policy(RefinmentStrategy::PartialShortCut(n_iterations)); }
    // refine_solution(strategy).  Reparent(radius) (pto_policy_refiner.rs:209-322) runs through porrt_bg_reparent_policy, with rules of
    // ours where the reference pins none: bit-equal queue priorities pop in ascending tree node id, a push replaces a queued node's
    // priority, and the options reparent_max_tree_nodes / reparent_max_pops_per_node cap a piece (PORRT_ERR_CAPACITY).  Its nodes are
    // belief-graph nodes: original_node_id and belief_state are each node's own, and a piece may come out longer than it went in.
    Policy refine_policy(const RefinmentStrategy &strategy) {
        Policy policy;
        auto call = [&](double *xy, uint64_t *oid, int64_t *par, uint8_t *leaf, uint64_t cap, double *cost) {
            return strategy.kind == RefinmentStrategy::kReparent ? porrt_bg_reparent_policy(ctx_.get(), strategy.radius, xy, oid, par, leaf, cap, cost)
                                                                 : porrt_bg_refine_policy(ctx_.get(), strategy.n_iterations, xy, oid, par, leaf, cap, cost);
        };
        const int64_t n = call(nullptr, nullptr, nullptr, nullptr, 0, nullptr);
        if (n < 0) ctx_.check((int)n);
        std::vector<double> xy(2 * (size_t)n);
        std::vector<uint64_t> oid((size_t)n);
        std::vector<int64_t> par((size_t)n);
        std::vector<uint8_t> leaf((size_t)n);
        const int64_t m = call(xy.data(), oid.data(), par.data(), leaf.data(), (uint64_t)n, &policy.expected_costs);
        if (m < 0) ctx_.check((int)m);
        const size_t nb = porrt_bg_num_beliefs(ctx_.get());
        std::vector<double> flat(nb * (size_t)n_worlds());
        ctx_.check(porrt_bg_get_beliefs(ctx_.get(), flat.data()));
        for (size_t k = 0; k < (size_t)n; ++k) {
            PolicyNode pn;
            pn.state = {xy[2 * k], xy[2 * k + 1]};
            pn.belief_state.assign(flat.begin() + (oid[k] % nb) * n_worlds(), flat.begin() + (oid[k] % nb + 1) * n_worlds());
            pn.original_node_id = (size_t)oid[k];
            if (par[k] >= 0) { pn.parent = (size_t)par[k]; policy.nodes[(size_t)par[k]].children.push_back(k); }
            policy.nodes.push_back(std::move(pn));
            if (leaf[k]) policy.leafs.push_back(k);
        }
        return policy;
    }
    // the same for every policy extract_policies() returned last, in one device call (porrt_bg_refine_policies): one refined Policy
    // per start, nullopt where there is none (statuses, when asked for: 1 no policy to refine, 2 a shortcut met a raster fault --
    // the reference panics --, 3 a piece whose nodes carry different beliefs -- the reference asserts)
    size_t n_policies_ = 0;                    // starts of the last extract_policies(): what porrt_bg_refine_policies answers for
    std::vector<std::optional<Policy>> refine_policies(size_t n_iterations, std::vector<uint8_t> *statuses = nullptr) {
        const int64_t cap = porrt_bg_get_policies(ctx_.get(), nullptr, nullptr, nullptr, 0);       // the nodes going in bound those coming out
        if (cap < 0) ctx_.check((int)cap);
        const size_t nq = n_policies_, room = (size_t)cap + 1;
        std::vector<uint64_t> off(nq + 1, 0), oid(room);
        std::vector<uint8_t> status(nq + 1, 0), leaf(room);
        std::vector<double> cost(nq + 1, 0.0), xy(2 * room);
        std::vector<int64_t> par(room);
        const int64_t n = porrt_bg_refine_policies(ctx_.get(), n_iterations, off.data(), status.data(), cost.data(), xy.data(), oid.data(), par.data(),
                                                   leaf.data(), (uint64_t)room);
        if (n < 0) ctx_.check((int)n);
        const size_t nb = porrt_bg_num_beliefs(ctx_.get()), nw = (size_t)n_worlds();
        std::vector<double> flat(nb * nw);
        ctx_.check(porrt_bg_get_beliefs(ctx_.get(), flat.data()));
        std::vector<std::optional<Policy>> out(nq);
        for (size_t q = 0; q < nq; ++q) {
            if (status[q]) continue;
            Policy policy;
            policy.expected_costs = cost[q];
            for (size_t k = 0, o = (size_t)off[q]; o < (size_t)off[q + 1]; ++k, ++o) {
                PolicyNode pn;
                pn.state = {xy[2 * o], xy[2 * o + 1]};
                pn.belief_state.assign(flat.begin() + (oid[o] % nb) * nw, flat.begin() + (oid[o] % nb + 1) * nw);
                pn.original_node_id = (size_t)oid[o];
                if (par[o] >= 0) { pn.parent = (size_t)par[o]; policy.nodes[(size_t)par[o]].children.push_back(k); }
                policy.nodes.push_back(std::move(pn));
                if (leaf[o]) policy.leafs.push_back(k);
            }
            out[q] = std::move(policy);
        }
        if (statuses) statuses->assign(status.begin(), status.begin() + nq);
        return out;
    }
    // pto.rs:151-183
    Policy plan_belief_space(const BeliefState &start_belief_state) {
        build_belief_graph_on_device(start_belief_state);
        compute_expected_costs_to_goals(false);
        return extract_policy();
    }
    // ---- QMdpPolicyExtractor (qmdp_policy_extractor.rs) on this graph
    // plan_qmdp :23-35; the costs stay on the device
    void plan_qmdp() { ctx_.check(porrt_qmdp_plan(ctx_.get())); }
    // cost_to_goals[world][node]
    std::vector<std::vector<double>> qmdp_cost_to_goals() const {
        const size_t n = (size_t)porrt_num_nodes(ctx_.get()), nw = (size_t)n_worlds();
        std::vector<double> flat(n * nw);
        ctx_.check(porrt_qmdp_get_costs(ctx_.get(), flat.data()));
        std::vector<std::vector<double>> out(nw);
        for (size_t w = 0; w < nw; ++w) out[w].assign(flat.begin() + w * n, flat.begin() + (w + 1) * n);
        return out;
    }
    // react_qmdp :38-49 for every query (start, belief, common horizon) in one call: result[q][world] is paths[world] of query q
    struct QmdpQuery { State start; BeliefState belief_state; double common_horizon; };
    std::vector<std::vector<std::vector<State>>> react_qmdp(const std::vector<QmdpQuery> &queries) {
        const size_t n = queries.size(), nw = (size_t)n_worlds();
        std::vector<double> s(2 * n), b(n * nw), h(n);
        for (size_t q = 0; q < n; ++q) {
            if (queries[q].belief_state.size() != nw) throw std::runtime_error("belief state size should match the number of worlds");
            s[2 * q] = queries[q].start[0]; s[2 * q + 1] = queries[q].start[1]; h[q] = queries[q].common_horizon;
            std::copy(queries[q].belief_state.begin(), queries[q].belief_state.end(), b.begin() + q * nw);
        }
        std::vector<uint64_t> off(n * nw + 1), common(n + 1);
        const int64_t total = porrt_qmdp_react(ctx_.get(), s.data(), b.data(), (uint32_t)nw, h.data(), (uint64_t)n, off.data(), common.data(), nullptr, 0);
        if (total < 0) ctx_.check((int)total);
        std::vector<double> xy(2 * (size_t)total + 2);
        if (total) {
            const int64_t r = porrt_qmdp_react(ctx_.get(), s.data(), b.data(), (uint32_t)nw, h.data(), (uint64_t)n, off.data(), common.data(), xy.data(), (uint64_t)total);
            if (r < 0) ctx_.check((int)r);
        }
        std::vector<std::vector<std::vector<State>>> paths(n, std::vector<std::vector<State>>(nw));
        for (size_t q = 0; q < n; ++q)
            for (size_t w = 0; w < nw; ++w)
                for (uint64_t k = off[q * nw + w]; k < off[q * nw + w + 1]; ++k) paths[q][w].push_back({xy[2 * k], xy[2 * k + 1]});
        return paths;
    }
    struct porrt_qmdp_info qmdp_info() const {
        struct porrt_qmdp_info i;
        ctx_.check(porrt_qmdp_info(ctx_.get(), &i));
        return i;
    }
    // get_policy_graph (qmdp_policy_extractor.rs:125-127, pto_graph.rs:363-419) after plan_qmdp: the graph pruned to the edges that
    // are the right decision under some belief.  keep / how: one byte per adjacency entry of the original graph in push order;
    // children[u] / parents[u]: the pruned lists in push order.
    struct PolicyGraph {
        std::vector<uint8_t> keep, how;
        std::vector<std::vector<uint32_t>> children, parents;
        struct porrt_policy_graph_info info;
    };
    PolicyGraph get_policy_graph() {
        ctx_.check(porrt_qmdp_policy_graph(ctx_.get()));
        PolicyGraph g;
        ctx_.check(porrt_qmdp_policy_graph_info(ctx_.get(), &g.info));
        const size_t n = (size_t)porrt_num_nodes(ctx_.get());
        g.keep.resize(g.info.entries + 1); g.how.resize(g.info.entries + 1);
        std::vector<uint64_t> coff(n + 1), poff(n + 1);
        std::vector<uint32_t> cid(g.info.kept + 1), pid(g.info.kept + 1);
        ctx_.check(porrt_qmdp_policy_graph_get(ctx_.get(), g.keep.data(), g.how.data(), coff.data(), cid.data(), poff.data(), pid.data()));
        g.keep.resize(g.info.entries); g.how.resize(g.info.entries);
        g.children.resize(n); g.parents.resize(n);
        for (size_t u = 0; u < n; ++u) {
            g.children[u].assign(cid.begin() + coff[u], cid.begin() + coff[u + 1]);
            g.parents[u].assign(pid.begin() + poff[u], pid.begin() + poff[u + 1]);
        }
        return g;
    }
    // the expansion without copying the lists to the host (plan_belief_space only needs the policy)
    void build_belief_graph_on_device(const BeliefState &start_belief_state) {
        ctx_.check(porrt_build_belief_graph(ctx_.get(), start_belief_state.data(), (uint32_t)start_belief_state.size()));
    }
private:
    Context ctx_;
    std::vector<uint64_t> reach_, final_ids_, final_masks_;
};

// dijkstra over PTOGraphWorldView (pto_graph.rs:245-303) of an explicit graph for every world at once (porrt_qmdp_costs):
// validities[node_validity[i]] is node i's word of world bits, children[i] its children in push order, finals[w] the final nodes
// of world w (none: that world's costs are all +inf).  Returns costs[world][node].
inline std::vector<std::vector<double>> qmdp_costs(const std::vector<State> &states, const std::vector<uint32_t> &node_validity,
                                                   const std::vector<uint64_t> &validities, const std::vector<std::vector<uint32_t>> &children,
                                                   const std::vector<std::vector<uint64_t>> &finals, int device = 0) {
    const size_t n = states.size(), nw = finals.size();
    std::vector<double> xy(2 * n), flat(n * nw);
    std::vector<uint64_t> coff(n + 1, 0), foff(nw + 1, 0), fid;
    std::vector<uint32_t> cid;
    for (size_t i = 0; i < n; ++i) {
        xy[2 * i] = states[i][0]; xy[2 * i + 1] = states[i][1];
        cid.insert(cid.end(), children[i].begin(), children[i].end());
        coff[i + 1] = cid.size();
    }
    for (size_t w = 0; w < nw; ++w) { fid.insert(fid.end(), finals[w].begin(), finals[w].end()); foff[w + 1] = fid.size(); }
    cid.push_back(0); fid.push_back(0);                      // (never read: keeps data() non-null for empty lists)
    const int r = porrt_qmdp_costs(device, (uint64_t)n, xy.data(), node_validity.data(), validities.data(), (uint32_t)validities.size(), (uint32_t)nw,
                                   coff.data(), cid.data(), foff.data(), fid.data(), flat.data());
    if (r != PORRT_OK) throw std::runtime_error("porrt_qmdp_costs failed (" + std::to_string(r) + ")");
    std::vector<std::vector<double>> out(nw);
    for (size_t w = 0; w < nw; ++w) out[w].assign(flat.begin() + w * n, flat.begin() + (w + 1) * n);
    return out;
}

// get_policy_graph (pto_graph.rs:363-419) of an explicit graph (porrt_policy_graph): children[i] in push order, costs[world][node]
// (+inf allowed).  Returns the pruned children lists; keep / how (one byte per adjacency entry in push order) and info on request.
inline std::vector<std::vector<uint32_t>> policy_graph(const std::vector<std::vector<uint32_t>> &children, const std::vector<std::vector<double>> &costs,
                                                       std::vector<uint8_t> *keep_out = nullptr, std::vector<uint8_t> *how_out = nullptr,
                                                       struct porrt_policy_graph_info *info = nullptr, int device = 0) {
    const size_t n = children.size(), nw = costs.size();
    std::vector<double> flat(n * nw + 1);
    std::vector<uint64_t> coff(n + 1, 0);
    std::vector<uint32_t> cid;
    for (size_t i = 0; i < n; ++i) { cid.insert(cid.end(), children[i].begin(), children[i].end()); coff[i + 1] = cid.size(); }
    for (size_t w = 0; w < nw; ++w) {
        if (costs[w].size() != n) throw std::runtime_error("policy_graph: costs[world][node], one value per node");
        std::copy(costs[w].begin(), costs[w].end(), flat.begin() + w * n);
    }
    const size_t ne = cid.size();
    cid.push_back(0);                                        // (never read: keeps data() non-null for empty lists)
    std::vector<uint8_t> keep(ne + 1), how(ne + 1);
    const int r = porrt_policy_graph(device, (uint64_t)n, (uint32_t)nw, coff.data(), cid.data(), flat.data(), keep.data(), how.data(), info);
    if (r != PORRT_OK) throw std::runtime_error("porrt_policy_graph failed (" + std::to_string(r) + ")");
    keep.resize(ne); how.resize(ne);
    std::vector<std::vector<uint32_t>> out(n);
    for (size_t i = 0; i < n; ++i)
        for (uint64_t k = coff[i]; k < coff[i + 1]; ++k) if (keep[k]) out[i].push_back(cid[k]);
    if (keep_out) *keep_out = keep;
    if (how_out) *how_out = how;
    return out;
}

// prm.rs:13-109.  init(start) + grow_graph(...) build one roadmap per call pair (porrt_grow_prm evaluates all samples at
// once; growing an existing roadmap further is a new call with the full iteration count on a sampler reset to its seed).
class PRM {
public:
    const Context &context() const { return ctx_; }          // (the drawing functions of MapShelfDomain / Map read the graph on its device)
    PTOGraph graph;
    size_t n_it = 0;
    PRM(const ContinuousSampler &cs, const GridDomain &fns, int device = 0) : ctx_(device) {
        ctx_.set_domain(fns);
        ctx_.check(porrt_set_sampler(ctx_.get(), cs.low.data(), cs.up.data(), cs.seed));
    }
    void init(State start) { start_ = start; }                                                        // prm.rs:33-36
    void grow_graph(double max_step, double search_radius, size_t n_iter) {                          // prm.rs:38-51
        ctx_.check(porrt_grow_prm(ctx_.get(), start_.data(), max_step, search_radius, n_iter));
        n_it += n_iter;
        const size_t n = porrt_num_nodes(ctx_.get());
        std::vector<double> xy(2 * n);
        ctx_.check(porrt_get_tree(ctx_.get(), xy.data(), nullptr, nullptr));
        uint64_t val[65];
        int nv = porrt_get_validities(ctx_.get(), val);
        graph.validities.assign(val, val + nv);
        graph.nodes.assign(n, PTONode{});
        for (size_t j = 0; j < n; ++j) { graph.nodes[j].state = {xy[2 * j], xy[2 * j + 1]}; graph.nodes[j].validity_id = 0; }
        const size_t E = porrt_num_edges(ctx_.get());
        std::vector<uint32_t> f(E), t(E), v(E);
        if (E) ctx_.check(porrt_get_edges(ctx_.get(), f.data(), t.data(), v.data()));
        for (size_t e0 = 0; e0 < E;) {             // prm.rs:96-103: neighbour -> new for all, then new -> neighbour; validity 0
            size_t e1 = e0;
            while (e1 < E && t[e1] == t[e0]) ++e1;
            for (size_t e = e0; e < e1; ++e) graph.add_edge(f[e], t[e], 0);
            for (size_t e = e0; e < e1; ++e) graph.add_edge(t[e], f[e], 0);
            e0 = e1;
        }
    }
    // prm.rs:111-123: empty when start and goal are not connected
    std::vector<State> plan_path(State start, State goal) {
        const int64_t n = porrt_prm_plan_path(ctx_.get(), start.data(), goal.data(), nullptr, 0);
        if (n < 0) ctx_.check((int)n);
        std::vector<double> xy(2 * (size_t)n);
        if (n) porrt_prm_plan_path(ctx_.get(), start.data(), goal.data(), xy.data(), (uint64_t)n);
        std::vector<State> path((size_t)n);
        for (size_t k = 0; k < (size_t)n; ++k) path[k] = {xy[2 * k], xy[2 * k + 1]};
        return path;
    }
    // plan_path for every (start, goal) pair in one call (porrt_prm_plan_paths): paths[i] == plan_path(queries[i].first, queries[i].second)
    std::vector<std::vector<State>> plan_paths(const std::vector<std::pair<State, State>> &queries) {
        const size_t n = queries.size();
        std::vector<double> s(2 * n), g(2 * n);
        for (size_t i = 0; i < n; ++i) {
            s[2 * i] = queries[i].first[0]; s[2 * i + 1] = queries[i].first[1];
            g[2 * i] = queries[i].second[0]; g[2 * i + 1] = queries[i].second[1];
        }
        std::vector<uint64_t> off(n + 1);
        const int64_t total = porrt_prm_plan_paths(ctx_.get(), s.data(), g.data(), (uint64_t)n, off.data(), nullptr, 0);
        if (total < 0) ctx_.check((int)total);
        std::vector<double> xy(2 * (size_t)total);
        if (total) {
            const int64_t r = porrt_prm_get_paths(ctx_.get(), xy.data(), (uint64_t)total);
            if (r < 0) ctx_.check((int)r);
        }
        std::vector<std::vector<State>> paths(n);
        for (size_t i = 0; i < n; ++i)
            for (uint64_t k = off[i]; k < off[i + 1]; ++k) paths[i].push_back({xy[2 * k], xy[2 * k + 1]});
        return paths;
    }
private:
    Context ctx_;
    State start_{0.0, 0.0};
};

// map_shelves_tamp_prm.rs:285-494.  plan() = grow_mm_prm, build_belief_graph, compute_expected_costs_to_goals, extract_policy
// (:310-326), all but the mode tree's bookkeeping on the device; refine_policy(n) = the reference driver's
// PTOPolicyRefiner::refine_solution(PartialShortCut(n)) of that policy (main.rs:546-575).
class MapShelfDomainTampPRM {
public:
    MapShelfDomainTampPRM(const ContinuousSampler &cs, const DiscreteSampler &ds, const MapShelfDomain &m, int device = 0) : ctx_(device) {
        ctx_.set_domain(m);
        ctx_.check(porrt_set_sampler(ctx_.get(), cs.low.data(), cs.up.data(), cs.seed));
        ctx_.check(porrt_set_discrete_seed(ctx_.get(), ds.seed));
    }
    Policy plan(State start, const BeliefState &initial_belief_state, double max_step, double search_radius, size_t n_iter_per_belief) {
        const int64_t r = porrt_mm_plan(ctx_.get(), start.data(), initial_belief_state.data(), (uint32_t)initial_belief_state.size(), max_step,
                                        search_radius, n_iter_per_belief);
        if (r < 0) ctx_.check((int)r);
        return fetch(false, 0);
    }
    Policy refine_policy(size_t n_iterations) { return fetch(true, n_iterations); }
    // plan() and refine_policy(refine_iterations) for many problems on this planner's map in one call (porrt_mm_plan_batch): plan p is
    // what a fresh planner seeded with seeds[p] = (continuous, discrete) gives.  This planner's own last plan is left as it is.
    // A plan without a policy (status != 0: 1 = the start has no finite expected cost) has no rows.
    struct BatchedPlan {
        uint8_t status = 0, refine_status = 0;
        double expected_costs = 0.0, refined_costs = 0.0;
        std::vector<State> states;                       // the refined policy's when refine_iterations > 0
        std::vector<uint64_t> original_node_ids;         // the plan's own belief node ids
        std::vector<int64_t> parents;                    // -1 = the root
        std::vector<uint8_t> is_leaf;
        porrt_mm_batch_plan counts{};
    };
    std::vector<BatchedPlan> plan_batch(const std::vector<State> &starts, const std::vector<BeliefState> &initial_belief_states,
                                        const std::vector<std::pair<uint64_t, uint64_t>> &seeds, double max_step, double search_radius,
                                        size_t n_iter_per_belief, size_t refine_iterations = 0) {
        const size_t n = starts.size();
        if (initial_belief_states.size() != n || seeds.size() != n) throw std::invalid_argument("plan_batch: one belief state and one seed pair per start");
        const size_t nw = n ? initial_belief_states[0].size() : 0;
        std::vector<double> s(2 * n), b(n * nw);
        std::vector<uint64_t> cs(n), ds(n), off(n + 1);
        for (size_t p = 0; p < n; ++p) {
            if (initial_belief_states[p].size() != nw) throw std::invalid_argument("plan_batch: belief states of one length");
            s[2 * p] = starts[p][0]; s[2 * p + 1] = starts[p][1];
            std::copy(initial_belief_states[p].begin(), initial_belief_states[p].end(), b.begin() + p * nw);
            cs[p] = seeds[p].first; ds[p] = seeds[p].second;
        }
        std::vector<uint8_t> st(n), rst(n);
        std::vector<double> cost(n), rcost(n);
        const int64_t total = porrt_mm_plan_batch(ctx_.get(), (uint32_t)n, s.data(), b.data(), cs.data(), ds.data(), (uint32_t)nw, max_step, search_radius,
                                                  n_iter_per_belief, refine_iterations, off.data(), st.data(), cost.data(), rst.data(), rcost.data(), nullptr,
                                                  nullptr, nullptr, nullptr, 0);
        if (total < 0) ctx_.check((int)total);
        std::vector<double> xy(2 * (size_t)total);
        std::vector<uint64_t> oid((size_t)total);
        std::vector<int64_t> par((size_t)total);
        std::vector<uint8_t> leaf((size_t)total);
        if (total) {
            const int64_t r = porrt_mm_plan_batch_get_policies(ctx_.get(), nullptr, xy.data(), oid.data(), par.data(), leaf.data(), (uint64_t)total);
            if (r < 0) ctx_.check((int)r);
        }
        std::vector<BatchedPlan> out(n);
        for (size_t p = 0; p < n; ++p) {
            BatchedPlan &o = out[p];
            o.status = st[p]; o.refine_status = rst[p]; o.expected_costs = cost[p]; o.refined_costs = rcost[p];
            for (uint64_t k = off[p]; k < off[p + 1]; ++k) {
                o.states.push_back({xy[2 * k], xy[2 * k + 1]});
                o.original_node_ids.push_back(oid[k]); o.parents.push_back(par[k]); o.is_leaf.push_back(leaf[k]);
            }
            ctx_.check(porrt_mm_plan_batch_get_plan(ctx_.get(), (uint32_t)p, &o.counts));
        }
        return out;
    }
    const Context &context() const { return ctx_; }
private:
    Policy fetch(bool refined, size_t n_iterations) {
        Policy policy;
        auto call = [&](double *xy, uint64_t *oid, int64_t *par, uint8_t *leaf, uint64_t cap) {
            return refined ? porrt_mm_refine_policy(ctx_.get(), n_iterations, xy, oid, par, leaf, cap, &policy.expected_costs)
                           : porrt_mm_extract_policy(ctx_.get(), oid, par, leaf, xy, cap, &policy.expected_costs);
        };
        const int64_t n = call(nullptr, nullptr, nullptr, nullptr, 0);
        if (n < 0) ctx_.check((int)n);
        std::vector<double> xy(2 * (size_t)n);
        std::vector<uint64_t> oid((size_t)n);
        std::vector<int64_t> par((size_t)n);
        std::vector<uint8_t> leaf((size_t)n);
        const int64_t m = call(xy.data(), oid.data(), par.data(), leaf.data(), (uint64_t)n);
        if (m < 0) ctx_.check((int)m);
        const size_t n_modes = porrt_mm_num_modes(ctx_.get()), nw = (size_t)porrt_n_worlds(ctx_.get());
        std::vector<uint64_t> off(n_modes + 1);
        ctx_.check(porrt_mm_bg_get_graph(ctx_.get(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, off.data(), nullptr));
        std::vector<BeliefState> beliefs(n_modes, BeliefState(nw));
        for (size_t k = 0; k < n_modes; ++k) {
            double rp = 0;
            uint64_t nn = 0, ne = 0, nf = 0;
            ctx_.check(porrt_mm_get_mode(ctx_.get(), k, beliefs[k].data(), &rp, &nn, &ne, &nf));
        }
        for (size_t k = 0; k < (size_t)n; ++k) {
            PolicyNode pn;
            pn.state = {xy[2 * k], xy[2 * k + 1]};
            const size_t mode = (size_t)(std::upper_bound(off.begin(), off.end(), oid[k]) - off.begin()) - 1;
            pn.belief_state = beliefs[mode];
            pn.original_node_id = (size_t)oid[k];
            if (par[k] >= 0) { pn.parent = (size_t)par[k]; policy.nodes[(size_t)par[k]].children.push_back(k); }
            policy.nodes.push_back(std::move(pn));
            if (leaf[k]) policy.leafs.push_back(k);
        }
        return policy;
    }
    Context ctx_;
};

enum class TampSearch { AStar, BranchAndBound, BranchAndBoundMultipleViewPoints };   // map_shelves_tamp_rrt.rs:67-71

// MapShelfDomainTampRRT (map_shelves_tamp_rrt.rs:135-291): plan(.., TampSearch::BranchAndBound) on the device
// (porrt_tamp_rrt_plan).  AStar and BranchAndBoundMultipleViewPoints throw: their expansion order cannot be
// pinned.  plan_astar (:432-563, porrt_tamp_rrt_plan_astar) is the former with equal priorities popped in
// ascending search node id.  plan_multiple_viewpoints (:293-430, porrt_tamp_rrt_plan_viewpoints) is the latter with the viewpoints
// of a query walked in ascending node id -- one of the orders the reference may take, which is why it is a method of its own.
// The stream mode, wave width and pool size are the context's options tamp_streams / tamp_wave / tamp_pool.
class MapShelfDomainTampRRT {
public:
    MapShelfDomainTampRRT(const ContinuousSampler &cs, const DiscreteSampler &ds, const MapShelfDomain &m, double goal_radius, int device = 0)
        : ctx_(device), goal_radius_(goal_radius) {
        ctx_.set_domain(m);
        ctx_.check(porrt_set_sampler(ctx_.get(), cs.low.data(), cs.up.data(), cs.seed));
        ctx_.check(porrt_set_discrete_seed(ctx_.get(), ds.seed));
    }
    Policy plan(State start, const BeliefState &initial_belief_state, double max_step, double search_radius, size_t n_iter_min,
                size_t n_iter_max, TampSearch search, uint32_t batch_K = 128) {
        if (search == TampSearch::BranchAndBoundMultipleViewPoints)
            throw std::runtime_error("MapShelfDomainTampRRT: TampSearch::BranchAndBoundMultipleViewPoints walks a HashSet; "
                                     "plan_multiple_viewpoints() offers it with the viewpoints in ascending node id");
        if (search == TampSearch::AStar)
            throw std::runtime_error("MapShelfDomainTampRRT: TampSearch::AStar's order among equal priorities cannot be pinned; "
                                     "plan_astar() offers it with ties popped in ascending search node id");
        if (search != TampSearch::BranchAndBound) throw std::runtime_error("MapShelfDomainTampRRT: only TampSearch::BranchAndBound is supported");
        const int64_t r = porrt_tamp_rrt_plan(ctx_.get(), start.data(), initial_belief_state.data(), (uint32_t)initial_belief_state.size(), max_step,
                                              search_radius, n_iter_min, n_iter_max, goal_radius_, batch_K);
        return read_policy(r, initial_belief_state.size());
    }
    // plan_branch_bound_multiple_viewpoints (:293-430), viewpoints in ascending node id.  max_viewpoints is ours, not the
    // reference's: 0 = all, n = the n cheapest solutions of every observation query.
    Policy plan_multiple_viewpoints(State start, const BeliefState &initial_belief_state, double max_step, double search_radius, size_t n_iter_min,
                                    size_t n_iter_max, uint32_t max_viewpoints = 0, uint32_t batch_K = 128) {
        const int64_t r = porrt_tamp_rrt_plan_viewpoints(ctx_.get(), start.data(), initial_belief_state.data(), (uint32_t)initial_belief_state.size(),
                                                         max_step, search_radius, n_iter_min, n_iter_max, goal_radius_, batch_K, max_viewpoints);
        return read_policy(r, initial_belief_state.size());
    }
    // plan_astar (:432-563) with bit-equal priorities popped in ascending search node id and a prior of positive entries only
    // (ours, not the reference's; porrt_tamp_rrt_plan_astar).  tamp_wave speculates, it never changes the result.
    Policy plan_astar(State start, const BeliefState &initial_belief_state, double max_step, double search_radius, size_t n_iter_min,
                      size_t n_iter_max, uint32_t batch_K = 128) {
        const int64_t r = porrt_tamp_rrt_plan_astar(ctx_.get(), start.data(), initial_belief_state.data(), (uint32_t)initial_belief_state.size(),
                                                    max_step, search_radius, n_iter_min, n_iter_max, goal_radius_, batch_K);
        return read_policy(r, initial_belief_state.size());
    }
    // plan_astar for many (start, prior, seed) on this planner's map in one device call (porrt_tamp_rrt_plan_astar_batch, DESIGN.md
    // section 25): plan p is, bit for bit, plan_astar alone with the continuous sampler seeded seeds[p] (seeds empty: this planner's
    // seed for every plan).  A plan without a path has status PORRT_ERR_NO_PATH in its record and an empty policy; it does not throw.
    struct AstarBatch {
        std::vector<Policy> policies;
        std::vector<porrt_tamp_batch_plan> plans;
        size_t n_ok = 0;
    };
    AstarBatch plan_astar_batch(const std::vector<State> &starts, const std::vector<BeliefState> &priors, const std::vector<uint64_t> &seeds,
                                double max_step, double search_radius, size_t n_iter_min, size_t n_iter_max, uint32_t batch_K = 128) {
        if (starts.size() != priors.size() || (!seeds.empty() && seeds.size() != starts.size()))
            throw std::runtime_error("MapShelfDomainTampRRT::plan_astar_batch: one start, one prior and (if any) one seed per plan");
        const size_t n = starts.size(), nw = n ? priors[0].size() : 0;
        std::vector<double> st, pr;
        for (size_t p = 0; p < n; ++p) {
            if (priors[p].size() != nw) throw std::runtime_error("MapShelfDomainTampRRT::plan_astar_batch: priors of different sizes");
            st.insert(st.end(), starts[p].begin(), starts[p].end());
            pr.insert(pr.end(), priors[p].begin(), priors[p].end());
        }
        const int64_t r = porrt_tamp_rrt_plan_astar_batch(ctx_.get(), (uint32_t)n, st.data(), pr.data(), seeds.empty() ? nullptr : seeds.data(),
                                                          (uint32_t)nw, max_step, search_radius, n_iter_min, n_iter_max, goal_radius_, batch_K);
        return read_batch<AstarBatch>(r, n, nw);
    }
    // plan(.., BranchAndBound) for many (start, prior, seed, discrete seed) on this planner's map in one device call
    // (porrt_tamp_rrt_plan_batch): plan p is, bit for bit, plan(.., BranchAndBound) alone on a fresh planner
    // whose continuous sampler is seeded seeds[p] and whose discrete sampler discrete_seeds[p] (seeds empty: this planner's seed for
    // every plan; discrete_seeds empty: seeds[p]).  This planner's own samplers are left alone.  A plan without a path has status
    // PORRT_ERR_NO_PATH in its record and an empty policy; it does not throw.
    struct Batch {
        std::vector<Policy> policies;
        std::vector<porrt_tamp_batch_plan> plans;
        std::vector<uint64_t> pruned;          // per plan: children not pushed
        size_t n_ok = 0;
    };
    Batch plan_batch(const std::vector<State> &starts, const std::vector<BeliefState> &priors, const std::vector<uint64_t> &seeds,
                     const std::vector<uint64_t> &discrete_seeds, double max_step, double search_radius, size_t n_iter_min, size_t n_iter_max,
                     uint32_t batch_K = 128) {
        if (starts.size() != priors.size() || (!seeds.empty() && seeds.size() != starts.size()) ||
            (!discrete_seeds.empty() && discrete_seeds.size() != starts.size()))
            throw std::runtime_error("MapShelfDomainTampRRT::plan_batch: one start, one prior and (if any) one seed and one discrete seed per plan");
        const size_t n = starts.size(), nw = n ? priors[0].size() : 0;
        std::vector<double> st, pr;
        for (size_t p = 0; p < n; ++p) {
            if (priors[p].size() != nw) throw std::runtime_error("MapShelfDomainTampRRT::plan_batch: priors of different sizes");
            st.insert(st.end(), starts[p].begin(), starts[p].end());
            pr.insert(pr.end(), priors[p].begin(), priors[p].end());
        }
        const int64_t r = porrt_tamp_rrt_plan_batch(ctx_.get(), (uint32_t)n, st.data(), pr.data(), seeds.empty() ? nullptr : seeds.data(),
                                                    discrete_seeds.empty() ? nullptr : discrete_seeds.data(), (uint32_t)nw, max_step, search_radius,
                                                    n_iter_min, n_iter_max, goal_radius_, batch_K);
        Batch out = read_batch<Batch>(r, n, nw);
        out.pruned.resize(n);
        for (size_t p = 0; p < n; ++p) ctx_.check(porrt_tamp_batch_get_pruned(ctx_.get(), (uint32_t)p, &out.pruned[p]));
        return out;
    }
    porrt_tamp_astar_info astar_info() const { porrt_tamp_astar_info i; ctx_.check(porrt_tamp_rrt_get_astar_info(ctx_.get(), &i)); return i; }
    porrt_tamp_info info() const { porrt_tamp_info i; ctx_.check(porrt_tamp_rrt_get_info(ctx_.get(), &i)); return i; }
    porrt_tamp_viewpoints_info viewpoints_info() const { porrt_tamp_viewpoints_info i; ctx_.check(porrt_tamp_rrt_get_viewpoints_info(ctx_.get(), &i)); return i; }
    const Context &context() const { return ctx_; }
private:
    Policy read_policy(int64_t r, size_t nw) {
        return read_policy(r, nw, [&](double *xy, int64_t *par, uint8_t *leaf, double *bel, uint64_t cap, double *cost) {
            return porrt_tamp_rrt_policy(ctx_.get(), xy, par, leaf, bel, cap, cost);
        });
    }
    // the records and policies of the batch call that returned r, of either search
    template <class BatchT>
    BatchT read_batch(int64_t r, size_t n, size_t nw) {
        if (r < 0) ctx_.check((int)r);
        BatchT out;
        out.n_ok = (size_t)r;
        out.policies.resize(n);
        out.plans.resize(n);
        for (size_t p = 0; p < n; ++p) {
            ctx_.check(porrt_tamp_batch_get_plan(ctx_.get(), (uint32_t)p, &out.plans[p]));
            if (out.plans[p].status != PORRT_OK) continue;
            const uint32_t plan = (uint32_t)p;
            out.policies[p] = read_policy((int64_t)out.plans[p].policy_nodes, nw, [&](double *xy, int64_t *par, uint8_t *leaf, double *bel, uint64_t cap, double *cost) {
                return porrt_tamp_batch_policy(ctx_.get(), plan, xy, par, leaf, bel, cap, cost);
            });
        }
        return out;
    }
    // fetch(xy, parents, is_leaf, beliefs, cap, expected_cost): porrt_tamp_rrt_policy, or a batch plan's porrt_tamp_batch_policy
    template <class Fetch>
    Policy read_policy(int64_t r, size_t nw, Fetch fetch) {
        if (r < 0) ctx_.check((int)r);
        const size_t n = (size_t)r;
        std::vector<double> xy(2 * n), bel(n * nw);
        std::vector<int64_t> par(n);
        std::vector<uint8_t> leaf(n);
        Policy policy;
        const int64_t m = fetch(xy.data(), par.data(), leaf.data(), bel.data(), (uint64_t)n, &policy.expected_costs);
        if (m < 0) ctx_.check((int)m);
        for (size_t k = 0; k < n; ++k) {
            PolicyNode pn;
            pn.state = {xy[2 * k], xy[2 * k + 1]};
            pn.belief_state.assign(bel.begin() + (ptrdiff_t)(k * nw), bel.begin() + (ptrdiff_t)((k + 1) * nw));
            pn.original_node_id = 0;
            policy.nodes.push_back(std::move(pn));
            if (par[k] >= 0) { policy.nodes[k].parent = (size_t)par[k]; policy.nodes[(size_t)par[k]].children.push_back(k); }
            if (leaf[k]) policy.leafs.push_back(k);
        }
        return policy;
    }
    Context ctx_;
    double goal_radius_;
};

} // namespace po_rrt
