// rq_topo.cpp -- graph topology and the controller's per-run tables (rq_host.h).
//
// topo_build does what SimOpts + Manager.__init__ + Broadcaster.init_state do in the
// reference (opt_model.py:145-181, :340-344, :773-780): validate the network, give every
// sink a dense column (sorted sink id order, the pivot_table column order of
// utils.py:54-55) and build the per-source sink lists in edge_list order (the
// Event.sink_ids of opt_model.py:306-307) as CSR.  rq_graph_build uploads the result.
#include <algorithm>
#include <cmath>
#include <unordered_map>
#include <vector>

#include "rq_host.h"

namespace rqh {

namespace {
constexpr int kBitsMaxSinks = 2048;   // bitset sweep: one 32-sink word per lane
}

int topo_build(const rq_graph_desc* d, GraphTopo* g)
{
    if (!d || !g) return RQ_EINVAL;
    if (d->n_sinks < 1 || !d->sink_ids) return RQ_EINVAL;              // "No sinks."
    if (d->n_sources < 0 || (d->n_sources > 0 && !d->sources)) return RQ_EINVAL;
    if (d->n_edges < 0 || (d->n_edges > 0 && (!d->edge_src || !d->edge_sink))) return RQ_EINVAL;
    if (!(d->end_time >= d->start_time)) return RQ_EINVAL;
    g->start = d->start_time;
    g->end = d->end_time;
    g->ctrl_src_id = d->ctrl_src_id;

    // sinks: dense columns in sorted id order; "Duplicates in sink_ids."
    std::vector<int64_t> sinks(d->sink_ids, d->sink_ids + d->n_sinks);
    std::sort(sinks.begin(), sinks.end());
    if (std::adjacent_find(sinks.begin(), sinks.end()) != sinks.end()) return RQ_EINVAL;
    g->n_sinks = d->n_sinks;
    g->sink_ids = sinks;
    std::unordered_map<int64_t, int> col;
    for (int c = 0; c < g->n_sinks; ++c) col[sinks[c]] = c;

    // sources: other sources + the controlled slot, in the order run_dynamic plays equal
    // times (opt_model.py:279-290): the dynamic sources (Poisson, Hawkes, a dynamic
    // broadcaster's replayed times) by src_id, then the static ones (Poisson2,
    // PiecewiseConst, RealData; the controlled slot -- a RedQueen controller's ties are
    // the sweep's cbf flags, the other controlled kinds are static) by src_id.  The merge
    // and the sequential sweep play equal times in stream order.
    struct S { int64_t id; int orig; int cls; };
    std::vector<S> order;
    for (int k = 0; k < d->n_sources; ++k) {
        const rq_source_desc& s = d->sources[k];
        if (s.kind < RQ_SRC_POISSON || s.kind > RQ_SRC_REALDATA) return RQ_EUNSUPPORTED;
        if ((s.flags & ~(uint32_t)RQ_SRCF_DYNAMIC) || ((s.flags & RQ_SRCF_DYNAMIC) && s.kind != RQ_SRC_REALDATA))
            return RQ_EINVAL;
        if (s.kind == RQ_SRC_PWCONST || s.kind == RQ_SRC_REALDATA) {
            if (s.n_arr < (s.kind == RQ_SRC_PWCONST ? 1 : 0) || (s.n_arr > 0 && !s.a)) return RQ_EINVAL;
            if (s.kind == RQ_SRC_PWCONST && !s.b) return RQ_EINVAL;
        }
        const bool stat = s.kind == RQ_SRC_POISSON2 || s.kind == RQ_SRC_PWCONST ||
                          (s.kind == RQ_SRC_REALDATA && !(s.flags & RQ_SRCF_DYNAMIC));
        order.push_back({s.src_id, k, stat ? 1 : 0});
    }
    order.push_back({d->ctrl_src_id, -1, 1});
    {
        std::vector<int64_t> ids;
        for (const S& o : order) ids.push_back(o.id);
        std::sort(ids.begin(), ids.end());
        if (std::adjacent_find(ids.begin(), ids.end()) != ids.end()) return RQ_EINVAL;   // "Duplicates in sources."
    }
    std::sort(order.begin(), order.end(),
              [](const S& x, const S& y) { return x.cls != y.cls ? x.cls < y.cls : x.id < y.id; });
    g->n_str = (int)order.size();
    std::unordered_map<int64_t, int> sidx;
    for (int j = 0; j < g->n_str; ++j) {
        const S& o = order[j];
        sidx[o.id] = j;
        g->src_id.push_back(o.id);
        g->orig_idx.push_back(o.orig);
        g->is_static.push_back(o.cls);
        g->arr_off.push_back((int)g->arr_a.size());
        if (o.orig < 0) {
            g->ctrl_idx = j;
            g->kind.push_back(RQ_SRC_NONE);
            g->seed.push_back(0);
            g->p0.push_back(0); g->p1.push_back(0); g->p2.push_back(0);
            g->ctrl_arr_off = (int)g->arr_a.size();
            int n = 0;
            if (d->ctrl_n_arr > 0 && d->ctrl_a) {
                std::vector<double> a(d->ctrl_a, d->ctrl_a + d->ctrl_n_arr);
                if (d->ctrl_b) {   // piecewise: keep order (asserted sorted)
                    if (!std::is_sorted(a.begin(), a.end())) return RQ_EINVAL;
                    for (int q = 0; q < d->ctrl_n_arr; ++q) {
                        g->arr_a.push_back(a[q]);
                        g->arr_b.push_back(d->ctrl_b[q]);
                    }
                    n = d->ctrl_n_arr;
                } else {           // real data: times in [start, end], sorted
                    std::vector<double> keep;
                    for (double t : a) if (t >= g->start && t <= g->end) keep.push_back(t);
                    std::sort(keep.begin(), keep.end());
                    for (double t : keep) { g->arr_a.push_back(t); g->arr_b.push_back(0.0); }
                    n = (int)keep.size();
                }
            }
            g->ctrl_arr_n = n;
            g->arr_n.push_back(n);
            continue;
        }
        const rq_source_desc& s = d->sources[o.orig];
        g->kind.push_back(s.kind);
        g->seed.push_back(s.seed);
        g->p0.push_back(s.p0); g->p1.push_back(s.p1); g->p2.push_back(s.p2);
        int n = 0;
        if (s.kind == RQ_SRC_PWCONST) {
            // PiecewiseConst asserts (opt_model.py:631, :644-645)
            if (!std::is_sorted(s.a, s.a + s.n_arr)) return RQ_EINVAL;
            if (s.a[0] != g->start || g->end < s.a[s.n_arr - 1]) return RQ_EINVAL;
            for (int q = 0; q < s.n_arr; ++q) { g->arr_a.push_back(s.a[q]); g->arr_b.push_back(s.b[q]); }
            n = s.n_arr;
        } else if (s.kind == RQ_SRC_REALDATA) {
            std::vector<double> keep;
            for (int q = 0; q < s.n_arr; ++q)
                if (s.a[q] >= g->start && s.a[q] <= g->end) keep.push_back(s.a[q]);
            std::sort(keep.begin(), keep.end());
            for (double t : keep) { g->arr_a.push_back(t); g->arr_b.push_back(0.0); }
            n = (int)keep.size();
        } else if (s.kind == RQ_SRC_HAWKES) {
            if (!(s.p0 >= 0.0) || !(s.p1 >= 0.0) || !(s.p2 >= 0.0)) return RQ_EINVAL;
        }
        g->arr_n.push_back(n);
    }

    {
        std::vector<double> tw, tc;
        for (int j = 0; j < g->n_str; ++j)
            if (g->kind[j] == RQ_SRC_REALDATA)
                tw.insert(tw.end(), g->arr_a.begin() + g->arr_off[j], g->arr_a.begin() + g->arr_off[j] + g->arr_n[j]);
        if (!d->ctrl_b)   // replayed controller times (change times of a piecewise one are not events)
            tc.assign(g->arr_a.begin() + g->ctrl_arr_off, g->arr_a.begin() + g->ctrl_arr_off + g->ctrl_arr_n);
        std::sort(tw.begin(), tw.end());
        g->rd_ties = std::adjacent_find(tw.begin(), tw.end()) != tw.end();
        tc.insert(tc.end(), tw.begin(), tw.end());
        std::sort(tc.begin(), tc.end());
        g->rd_ties_ctrl = std::adjacent_find(tc.begin(), tc.end()) != tc.end();
    }

    // edges: "Unknown sources/sinks in edge_list." ; CSR in edge-list order
    std::vector<std::vector<int>> rows(g->n_str);
    for (int64_t e = 0; e < d->n_edges; ++e) {
        auto si = sidx.find(d->edge_src[e]);
        auto ci = col.find(d->edge_sink[e]);
        if (si == sidx.end() || ci == col.end()) return RQ_EINVAL;
        rows[si->second].push_back(ci->second);
    }
    g->n_edges = d->n_edges;
    // followers of the controlled source: sorted distinct sink order (Opt.sink_ids,
    // opt_model.py:341, as the State's follower ranks key them)
    std::vector<int> fcols = rows[g->ctrl_idx];
    std::sort(fcols.begin(), fcols.end());
    g->ctrl_dup = std::adjacent_find(fcols.begin(), fcols.end()) != fcols.end();
    fcols.erase(std::unique(fcols.begin(), fcols.end()), fcols.end());
    g->n_fol = (int)fcols.size();
    g->col_to_fol.assign(g->n_sinks, -1);
    for (int f = 0; f < g->n_fol; ++f) {
        g->col_to_fol[fcols[f]] = f;
        g->fol_ids.push_back(sinks[fcols[f]]);
    }
    g->fol = fcols;
    g->csr_ptr.push_back(0);
    g->lay_ptr.push_back(0);
    std::vector<int> seen(g->n_sinks, 0);
    for (int j = 0; j < g->n_str; ++j) {
        // layer k holds the (k+1)-th occurrence of each sink, in edge-list order; the
        // controlled row's layer 0 is the sorted follower list the sweep indexes by
        // follower position
        std::vector<std::vector<int>> layers;
        for (int c : rows[j]) {
            const int k = seen[c]++;
            if ((int)layers.size() <= k) layers.emplace_back();
            layers[k].push_back(c);
        }
        for (int c : rows[j]) seen[c] = 0;
        if (j == g->ctrl_idx && !layers.empty()) layers[0] = fcols;
        g->multi = g->multi || layers.size() > 1;
        int of = 0;
        for (const std::vector<int>& l : layers) {
            for (int c : l) {
                g->csr_col.push_back(c);
                of += g->col_to_fol[c] >= 0;
            }
            g->lay_end.push_back((int)g->csr_col.size());
        }
        if (layers.empty()) g->lay_end.push_back((int)g->csr_col.size());
        g->lay_ptr.push_back((int)g->lay_end.size());
        g->outdeg_f.push_back(of);
        g->csr_ptr.push_back((int)g->csr_col.size());
        // dataframe export: every stream's sinks in edge-list order (duplicates included:
        // Event.sink_ids, opt_model.py:306-307)
        for (int c : rows[j]) g->csr_col_el.push_back(c);
    }

    if (g->n_sinks <= kBitsMaxSinks) {
        g->nw = (g->n_sinks + 31) / 32;
        g->masks.assign((size_t)g->n_str * g->nw, 0u);
        for (int j = 0; j < g->n_str; ++j)
            for (int e = g->csr_ptr[j]; e < g->csr_ptr[j + 1]; ++e) {
                const int c = g->csr_col[e];
                g->masks[(size_t)j * g->nw + c / 32] |= 1u << (c % 32);
            }
    }

    g->fbits.assign((g->n_sinks + 31) / 32, 0u);
    for (int c : g->fol) g->fbits[c / 32] |= 1u << (c % 32);
    g->cbf.resize(g->n_str);
    for (int j = 0; j < g->n_str; ++j) g->cbf[j] = g->is_static[j] || g->ctrl_src_id < g->src_id[j];

    // the generator's class lists: Hawkes, then the Poisson kinds, then the rest, each in
    // stream order; the controlled slot joins its call's class at the launch
    g->gen_cls.clear();
    for (int c = 0; c < 3; ++c) {
        g->gen_n[c] = 0;
        for (int j = 0; j < g->n_str; ++j) {
            if (j == g->ctrl_idx) continue;
            const int k = g->kind[j];
            const int cj = k == RQ_SRC_HAWKES ? 0 : (k == RQ_SRC_POISSON || k == RQ_SRC_POISSON2) ? 1 : 2;
            if (cj != c) continue;
            g->gen_cls.push_back(j);
            ++g->gen_n[c];
        }
    }

    // the sink-tiled CSR (rq_host.h): a stable counting sort of the edges by (tile, stream)
    if (!g->multi && g->n_sinks <= RQ_FOLLOWERS_TILED_MAX_SINKS) {
        const int TS = RQ_FOLLOWERS_TILE_SINKS;
        const int nt = followers_tiles(g->n_sinks);
        const size_t stride = (size_t)g->n_str + 1;
        g->n_tiles = nt;
        g->tile_ptr.assign((size_t)nt * stride, 0);
        g->tile_col.resize(g->csr_col_el.size());
        std::vector<int> at((size_t)nt * g->n_str, 0);   // counts, then write cursors
        for (int j = 0; j < g->n_str; ++j)
            for (int e = g->csr_ptr[j]; e < g->csr_ptr[j + 1]; ++e)
                ++at[(size_t)(g->csr_col_el[e] / TS) * g->n_str + j];
        int off = 0;
        for (int i = 0; i < nt; ++i) {
            for (int j = 0; j < g->n_str; ++j) {
                g->tile_ptr[i * stride + j] = off;
                const int n = at[(size_t)i * g->n_str + j];
                at[(size_t)i * g->n_str + j] = off;
                off += n;
            }
            g->tile_ptr[i * stride + g->n_str] = off;
        }
        for (int j = 0; j < g->n_str; ++j)
            for (int e = g->csr_ptr[j]; e < g->csr_ptr[j + 1]; ++e) {
                const int c = g->csr_col_el[e];
                g->tile_col[at[(size_t)(c / TS) * g->n_str + j]++] = c;
            }
    }
    return RQ_OK;
}

CtrlTables ctrl_tables(const GraphTopo& g, const rq_batch_desc* b)
{
    CtrlTables t;
    // c_j = sum over edges (j, i), i a follower, of sqrt(s_i / q)  (opt_model.py:515, :536)
    t.invc.assign((size_t)b->n_grid * g.n_str, 0.0);
    if (b->ctrl_kind == RQ_SRC_OPT) {
        std::vector<double> w(g.n_fol);
        for (int gi = 0; gi < b->n_grid; ++gi) {
            for (int f = 0; f < g.n_fol; ++f) w[f] = std::sqrt(b->s[(size_t)gi * g.n_fol + f] / b->q[gi]);
            for (int j = 0; j < g.n_str; ++j) {
                if (j == g.ctrl_idx) continue;
                double c = 0.0;
                // edge-list order (duplicate edges count once each), as the oracle sums
                for (int e = g.csr_ptr[j]; e < g.csr_ptr[j + 1]; ++e) {
                    const int f = g.col_to_fol[g.csr_col_el[e]];
                    if (f >= 0) c = c + w[f];
                }
                t.invc[(size_t)gi * g.n_str + j] = c > 0.0 ? 1.0 / c : 0.0;
            }
        }
    }
    // OptPWSignificance: per (grid point, stream) the intensity increment of one event
    // of stream j per significance segment, pw[k] = sum over edges (j, i), i a follower,
    // of sqrt(s_pw[i, k] / q) (opt_model.py:613-614 with rank_diff_i = edge multiplicity),
    // edge-list order; and its max over k (the thinning bound, :563)
    if (b->ctrl_kind == RQ_SRC_OPTPW) {
        const int S = b->n_seg;
        t.pwc.assign((size_t)b->n_grid * g.n_str * S, 0.0);
        t.pwmax.assign((size_t)b->n_grid * g.n_str, 0.0);
        for (int gi = 0; gi < b->n_grid; ++gi)
            for (int j = 0; j < g.n_str; ++j) {
                if (j == g.ctrl_idx) continue;
                double* row = &t.pwc[((size_t)gi * g.n_str + j) * S];
                for (int e = g.csr_ptr[j]; e < g.csr_ptr[j + 1]; ++e) {
                    const int f = g.col_to_fol[g.csr_col_el[e]];
                    if (f < 0) continue;
                    const double* sp = b->s_pw + ((size_t)gi * g.n_fol + f) * S;
                    for (int k = 0; k < S; ++k) row[k] = row[k] + std::sqrt(sp[k] / b->q[gi]);
                }
                double m = 0.0;
                for (int k = 0; k < S; ++k) m = row[k] > m ? row[k] : m;
                t.pwmax[(size_t)gi * g.n_str + j] = m;
            }
    }
    return t;
}

int game_tables(const GraphTopo& g, const rq_game_player* players, int n_players, GameTables* out)
{
    if (!players || !out || n_players < 1) return RQ_EINVAL;
    if (n_players > RQ_GAME_MAX_PLAYERS) return RQ_EUNSUPPORTED;
    const int P = n_players;
    struct L { int64_t id; int col, stream; };
    std::vector<L> lanes;
    for (int c = 0; c < P; ++c) {
        const rq_game_player& p = players[c];
        int j = -1;
        for (int k = 0; k < g.n_str; ++k)
            if (g.src_id[k] == p.src_id) j = k;
        if (j < 0) return RQ_EINVAL;   // not a stream of the graph
        // a replay stream: the controlled slot, or a dynamic RealData source without times
        const bool replay = j == g.ctrl_idx ||
                            (g.kind[j] == RQ_SRC_REALDATA && !g.is_static[j] && g.arr_n[j] == 0);
        if (!replay) return RQ_EINVAL;
        if (!(p.q > 0.0) || p.n_s < 1 || !p.s) return RQ_EINVAL;
        lanes.push_back({p.src_id, c, j});
    }
    std::sort(lanes.begin(), lanes.end(), [](const L& a, const L& b) { return a.id < b.id; });
    for (int c = 1; c < P; ++c)
        if (lanes[c].id == lanes[c - 1].id) return RQ_EINVAL;   // a player named twice

    GameTables t;
    t.P = P;
    t.C.assign((size_t)P * g.n_str, 0.0);
    t.inv.assign((size_t)g.n_str * P, 0.0);
    std::vector<double> w(g.n_sinks);
    std::vector<int> row;
    for (int c = 0; c < P; ++c) {
        const rq_game_player& p = players[lanes[c].col];
        const int jc = lanes[c].stream;
        t.lane_stream.push_back(jc);
        t.lane_col.push_back(lanes[c].col);
        if (jc == g.ctrl_idx) t.ctrl_lane = c;
        // the player's followers: the distinct sinks of its edges, ascending (columns are in
        // ascending sink id); a duplicated own edge is the reference's shape error
        std::vector<int> fc(g.csr_col_el.begin() + g.csr_ptr[jc], g.csr_col_el.begin() + g.csr_ptr[jc + 1]);
        std::sort(fc.begin(), fc.end());
        if (fc.empty()) return RQ_EINVAL;
        if (std::adjacent_find(fc.begin(), fc.end()) != fc.end()) return RQ_EINVAL;
        if ((int)fc.size() != p.n_s) return RQ_EINVAL;
        std::fill(w.begin(), w.end(), -1.0);   // -1: no follower of c
        for (int f = 0; f < p.n_s; ++f) {
            if (!(p.s[f] >= 0.0)) return RQ_EINVAL;
            w[fc[f]] = std::sqrt(p.s[f] / p.q);
        }
        for (int j = 0; j < g.n_str; ++j) {
            if (j == jc) continue;
            row.assign(g.csr_col_el.begin() + g.csr_ptr[j], g.csr_col_el.begin() + g.csr_ptr[j + 1]);
            std::sort(row.begin(), row.end());   // ascending sink id, duplicates kept
            double cj = 0.0;
            for (int x : row)
                if (w[x] >= 0.0) cj = cj + w[x];
            t.C[(size_t)c * g.n_str + j] = cj;
            t.inv[(size_t)j * P + c] = cj > 0.0 ? 1.0 / cj : 0.0;
        }
    }
    t.meta.assign(g.n_str, 0);
    for (int j = 0; j < g.n_str; ++j) {
        // the controlled slot counts as static (is_static): in an exogenous log it is a
        // static controller's stream
        int first = P;
        if (!g.is_static[j]) {
            first = 0;
            for (int c = 0; c < P; ++c) first += lanes[c].id < g.src_id[j];
        }
        t.meta[j] = first | (g.csr_ptr[j + 1] > g.csr_ptr[j] ? RQ_GAME_META_EDGE : 0);
    }
    *out = std::move(t);
    return RQ_OK;
}

int log_of_streams(const GraphTopo& g, const int64_t* src_ids, int n_src, int* trk)
{
    if (!src_ids || !trk || n_src < 1 || n_src > RQ_LOG_OF_MAX_SRC) return RQ_EINVAL;
    for (int k = 0; k < n_src; ++k) {
        int j = -1;
        for (int q = 0; q < g.n_str; ++q)
            if (g.src_id[q] == src_ids[k]) j = q;
        if (j < 0) return RQ_EINVAL;   // not a stream of the graph
        for (int q = 0; q < k; ++q)
            if (trk[q] == j) return RQ_EINVAL;   // named twice
        trk[k] = j;
    }
    return RQ_OK;
}

}  // namespace rqh
