// C ABI (include/jrr.h), jrr_model_*: the body model re-laid out on the host for the kernels (jrr_common.h struct Model) and uploaded.
#include <algorithm>
#include <array>
#include <cstring>
#include <tuple>
#include <vector>

#include "engine.h"

using namespace jrr;

constexpr int MAX_FACES = 14336;       // the rasteriser's capacity: 1024 threads x 14 faces (sil.hip)

// The model buffer: float / int32 tables back to back in this order (sizes in 4-byte words), then the face tables.
constexpr size_t nDk = (size_t)VT * KFP * 96, nDn = (size_t)3 * VP * KFP, nDq = nDn, nWjv = (size_t)VT * NJ * 32, nWvj = (size_t)VT * 1024;
constexpr size_t nJt = 72 + 24, nJS = 720 + 16;   // padded to keep 16-byte alignment of what follows
constexpr size_t nWc = (size_t)(VT + 1) * NJ * 32, nJl = (size_t)VT * NJ + (size_t)VT + 8, nPerm = (size_t)VP + 6912;   // jl [VT][24] + tnj [VT] (+ pad); p2v [VP], v2p [V] padded
constexpr size_t nW16 = (size_t)VT * 16 * 36, nSeg = (size_t)VT * 32;                      // segid [VT] (padded to 16 per tile), segj [VT][16]
constexpr size_t MODEL_FLOATS = nDk + nDn + nDq + nWjv + nWvj + nJt + nJS + nWc + nJl + nPerm + nW16 + nSeg;

// the tables of one buffer, host or device
struct Tables {
  float *Dk, *Dn, *Dq, *Wjv, *Wvj, *Jt, *JS, *Wc;
  int32_t *Jl, *Tnj, *P2V, *V2P;
  float* W16;
  int32_t *SegId, *SegJ;
  explicit Tables(float* b) {
    Dk = b; Dn = Dk + nDk; Dq = Dn + nDn; Wjv = Dq + nDq; Wvj = Wjv + nWjv; Jt = Wvj + nWvj; JS = Jt + nJt; Wc = JS + nJS;
    Jl = reinterpret_cast<int32_t*>(Wc + nWc); Tnj = Jl + (size_t)VT * NJ; P2V = Jl + nJl; V2P = P2V + VP;
    W16 = reinterpret_cast<float*>(P2V + nPerm);
    SegId = reinterpret_cast<int32_t*>(W16 + nW16); SegJ = SegId + (size_t)VT * 16;
  }
};

extern "C" size_t jrr_model_bytes(void) { return round_up(MODEL_FLOATS * sizeof(float), 256) + (size_t)2 * MAX_FACES * (3 + 2) * sizeof(int32_t); }

// =============================================================================================
// step 1: the internal vertex order (jrr_common.h)
// =============================================================================================
constexpr long COST_NO_FIT = (long)1 << 40;
// cost of an order for the joint-sparse kernels: matrix instructions of the forward kernel with per-tile classes (a tile
// above the slot count pays a second pass), COST_NO_FIT when a tile exceeds the backward kernel's 16-joint window
static long order_cost(const float* W, const std::vector<int>& order) {
  long cost8 = 0, cost12 = 0;
  for (int t = 0; t < VT; ++t) {
    bool used[NJ] = {false};
    for (int vv = 0; vv < 32; ++vv) {
      const int p_ = t * 32 + vv;
      if (p_ >= V) break;
      for (int j = 0; j < NJ; ++j) used[j] = used[j] || W[(size_t)order[p_] * NJ + j] != 0.f;
    }
    int n = 0;
    for (int j = 0; j < NJ; ++j) n += used[j];
    if (n > KJS_TILE_MAX) return COST_NO_FIT;
    cost8 += 423 + (n > 8 ? 78 : 0);
    cost12 += 447 + (n > 12 ? 102 : 0);
  }
  return std::min(cost8, cost12);
}

// joints of each vertex by descending weight (dominant joint first), NJ = none
static std::vector<std::array<int, 4>> dominant_joints(const float* W) {
  std::vector<std::array<int, 4>> inf4(V);
  for (int v = 0; v < V; ++v) {
    std::vector<std::pair<float, int>> inf;
    for (int j = 0; j < NJ; ++j) if (W[(size_t)v * NJ + j] != 0.f) inf.push_back({-W[(size_t)v * NJ + j], j});
    std::sort(inf.begin(), inf.end());
    for (int k = 0; k < 4; ++k) inf4[v][k] = k < (int)inf.size() ? inf[k].second : NJ;
  }
  return inf4;
}

// Sort keys along the KINEMATIC CHAINS: body parts (dominant joint) in depth-first order of the skeleton, so that neighbouring
// parts share joints; inside a part the vertices also tied to the previous part first, those tied to the next part last,
// the rest by their other joints.  A tile that straddles two parts then sees few joints beyond either part's own
// (capsule body in a random file order: 0 of 216 tiles above 8 joints, mean 4.4 -- the lexicographic order: 4, mean 4.8)
static std::vector<std::array<int, 6>> chain_keys(const std::vector<std::array<int, 4>>& inf4, const int32_t* parents) {
  std::vector<int> dfs, pos(NJ + 1, NJ);
  {
    std::vector<int> stack{0};
    while (!stack.empty()) {
      const int j = stack.back(); stack.pop_back();
      dfs.push_back(j);
      for (int q = NJ - 1; q > j; --q) if (parents[q] == j) stack.push_back(q);      // children in ascending order
    }
    for (int i = 0; i < (int)dfs.size(); ++i) pos[dfs[i]] = i;
  }
  std::vector<std::array<int, 6>> ckey(V);
  for (int v = 0; v < V; ++v) {
    const int p0 = pos[inf4[v][0]];
    const int prev_j = p0 > 0 ? dfs[p0 - 1] : -1, next_j = p0 + 1 < (int)dfs.size() ? dfs[p0 + 1] : -1;
    bool has_prev = false, has_next = false;
    std::array<int, 3> sec{NJ, NJ, NJ};
    for (int k = 1; k < 4; ++k) {
      const int j = inf4[v][k];
      if (j == NJ) continue;
      has_prev = has_prev || j == prev_j; has_next = has_next || j == next_j;
      sec[k - 1] = pos[j];
    }
    std::sort(sec.begin(), sec.end());
    ckey[v] = {p0, (has_prev && !has_next) ? 0 : (has_next && !has_prev) ? 2 : 1, sec[0], sec[1], sec[2], v};
  }
  return ckey;
}

// HINT (jrr_model_create_hinted): the vertices the caller's regressor will read -- its support -- are stored FIRST, packed into
// as few tiles as the joint-sparse kernels like: groups of hinted vertices along the kinematic chains whose joints number at
// most 8 (one pass of the 8-slot kernels), each group topped up to a full tile with other vertices of the same joints; the
// rest follows in `order`.  The iterations of JRR_FLAG_SUPPORT_TILES then run one tile per group instead of up to one per
// support entry.  Returns the distinct hinted vertices placed, 0 (and `order` as it was) when a group cannot be completed
// within the 16-joint window.
static int apply_hint(const float* W, const std::vector<std::array<int, 6>>& ckey, const int32_t* hint_vertices, int n_hint, std::vector<int>& order) {
  std::vector<char> is_hint(V, 0), used(V, 0);
  std::vector<int> hinted;
  for (int i = 0; i < n_hint; ++i) if (!is_hint[hint_vertices[i]]) { is_hint[hint_vertices[i]] = 1; hinted.push_back(hint_vertices[i]); }
  std::sort(hinted.begin(), hinted.end(), [&](int x, int y) { return ckey[x] < ckey[y]; });
  auto joints_of = [&](int v) { unsigned m_ = 0; for (int j = 0; j < NJ; ++j) if (W[(size_t)v * NJ + j] != 0.f) m_ |= 1u << j; return m_; };
  std::vector<int> with_hint;
  bool ok = true;
  size_t at = 0;
  while (at < hinted.size() && ok) {
    unsigned uni = 0;
    std::vector<int> tile;
    while (at < hinted.size() && tile.size() < 32) {      // the next group: joints <= 8 (a single vertex may bring up to 4)
      const unsigned grown = uni | joints_of(hinted[at]);
      if (!tile.empty() && __builtin_popcount(grown) > 8) break;
      uni = grown; tile.push_back(hinted[at]); used[hinted[at]] = 1; ++at;
    }
    for (int limit : {0, 8, KJS_TILE_MAX}) {               // fillers: joints inside the group's, then anything that keeps <= 8, <= 16
      for (int v : order) {
        if (tile.size() == 32) break;
        if (used[v] || is_hint[v]) continue;
        const unsigned grown = uni | joints_of(v);
        if (limit == 0 ? grown != uni : __builtin_popcount(grown) > limit) continue;
        uni = grown; tile.push_back(v); used[v] = 1;
      }
      if (tile.size() == 32) break;
    }
    ok = tile.size() == 32;
    with_hint.insert(with_hint.end(), tile.begin(), tile.end());
  }
  if (!ok) return 0;
  for (int v : order) if (!used[v]) with_hint.push_back(v);
  if ((int)with_hint.size() != V || order_cost(W, with_hint) >= COST_NO_FIT) return 0;
  order = with_hint;
  return (int)hinted.size();
}

// The file order unless it does not fit the joint-sparse kernels and a joint-sorted order does (or `force` asks for it:
// JRR_VERTEX_ORDER=sorted, tests), then the caller's hint.  order[row] = vertex of the file.
struct VertexOrder { std::vector<int> order; bool permuted = false; int hint_applied = 0; };
static VertexOrder choose_vertex_order(const float* W, const int32_t* parents, const int32_t* hint_vertices, int n_hint, bool force) {
  VertexOrder o;
  o.order.resize(V);
  for (int v = 0; v < V; ++v) o.order[v] = v;
  const long cost_file = order_cost(W, o.order);
  if (!(force || n_hint > 0 || cost_file > (long)VT * 423)) return o;      // no tile of the file order is wide
  // would a joint-sorted order be cheaper?  (a) lexicographic: (dominant joint, second, third, fourth, file index); (b) chain_keys
  const std::vector<std::array<int, 4>> inf4 = dominant_joints(W);
  std::vector<int> lex(o.order);
  std::sort(lex.begin(), lex.end(), [&](int a, int b) { return std::tie(inf4[a], a) < std::tie(inf4[b], b); });
  const std::vector<std::array<int, 6>> ckey = chain_keys(inf4, parents);
  std::vector<int> chain(o.order);
  std::sort(chain.begin(), chain.end(), [&](int a, int b) { return ckey[a] < ckey[b]; });
  const long cost_lex = order_cost(W, lex), cost_chain = order_cost(W, chain);
  if (force || std::min(cost_chain, cost_lex) < cost_file) { o.order = cost_chain <= cost_lex ? chain : lex; o.permuted = true; }
  if (n_hint > 0) {
    o.hint_applied = apply_hint(W, ckey, hint_vertices, n_hint, o.order);
    if (o.hint_applied) o.permuted = true;
  }
  return o;
}

// =============================================================================================
// step 2: joint-sparse skinning tables (jrr_common.h): per 32-vertex tile the joints with a non-zero weight.  PER-TILE classes: the
// kernels are built for `kjs` (8 or 12) joint slots per tile and pass; a tile with more joints (up to KJS_TILE_MAX = 16:
// the backward kernel's joint windows) costs ITSELF a second pass over slots kjs .. 2 kjs - 1, nobody else anything.
// =============================================================================================
struct TileClasses {
  std::vector<std::vector<int>> lists;      // [VT] the tile's joints, ascending
  int kjs = 0, wide_tiles = 0, most_joints = 0;
  int hist[NJ + 1] = {0};                   // tiles by joint count
};
static TileClasses classify_tiles(const float* W, const std::vector<int>& order, const Knobs& kn) {
  TileClasses c;
  c.lists.resize(VT);
  size_t most = 0;
  for (int t = 0; t < VT; ++t) {
    for (int j = 0; j < NJ; ++j) {
      bool used = false;
      for (int vv = 0; vv < 32 && !used; ++vv) { const int p_ = t * 32 + vv; used = p_ < V && W[(size_t)order[p_] * NJ + j] != 0.f; }
      if (used) c.lists[t].push_back(j);
    }
    most = std::max(most, c.lists[t].size());
    ++c.hist[c.lists[t].size()];
  }
  c.most_joints = (int)most;
  if (most <= (size_t)KJS_TILE_MAX) {
    // matrix instructions per tile of the forward kernel: 423 / 447 with 8 / 12 slots, + one pass (2 kjs x 3 + ~3 stage
    // hand-overs) for a wide tile
    long cost8 = 0, cost12 = 0;
    for (int t = 0; t < VT; ++t) {
      cost8 += 423 + (c.lists[t].size() > 8 ? 48 + 30 : 0);
      cost12 += 447 + (c.lists[t].size() > 12 ? 72 + 30 : 0);
    }
    c.kjs = cost8 <= cost12 ? 8 : KJS_MAX;
  }
  // JRR_DENSE_SKINNING=1 forces the dense kernels, JRR_SKIN_JOINTS=12 the 12-slot variant (verification: tests)
  if (kn.dense_skinning) c.kjs = 0;
  if (kn.skin_joints_12 && c.kjs == 8) c.kjs = 12;
  for (int t = 0; t < VT && c.kjs; ++t) c.wide_tiles += (int)c.lists[t].size() > c.kjs;
  return c;
}
// jl / tnj / Wc: NJ slots per tile
static void build_tile_lists(const float* W, const std::vector<int>& order, const TileClasses& c, Tables& h) {
  for (int t = 0; t < VT; ++t) {
    h.Tnj[t] = (int)c.lists[t].size();
    for (int n = 0; n < NJ; ++n) {                                     // NJ slots per tile: the tile's joints, ascending, then padding
      const int j = n < (int)c.lists[t].size() ? c.lists[t][n] : 0;    // padding: joint 0 with zero weights
      h.Jl[t * NJ + n] = j;
      for (int vv = 0; vv < 32; ++vv) {
        const int p_ = t * 32 + vv;
        h.Wc[((size_t)t * NJ + n) * 32 + vv] = (n < (int)c.lists[t].size() && p_ < V) ? W[(size_t)order[p_] * NJ + j] : 0.f;
      }
    }
  }
}

// =============================================================================================
// step 3: segments for the backward kernel's 16-row dA windows (segid / segj / W16): greedy runs of tiles whose joint union stays <= 16
// =============================================================================================
static void build_backward_windows(const float* W, const std::vector<int>& order, const std::vector<std::vector<int>>& lists, Tables& h) {
  int seg = 0;
  std::vector<int> win;      // joints of the current segment, in order of first appearance
  std::vector<int> first_tile{0};
  for (int t = 0; t < VT; ++t) {
    std::vector<int> grown(win);
    for (int j : lists[t]) if (std::find(grown.begin(), grown.end(), j) == grown.end()) grown.push_back(j);
    if (grown.size() > 16) {   // close the segment: its window is final
      for (int u = first_tile[seg]; u < t; ++u) for (int n = 0; n < 16; ++n) h.SegJ[u * 16 + n] = n < (int)win.size() ? win[n] : -1;
      ++seg; first_tile.push_back(t);
      win = lists[t];
    } else win = grown;
    h.SegId[t] = seg;
  }
  for (int u = first_tile[seg]; u < VT; ++u) for (int n = 0; n < 16; ++n) h.SegJ[u * 16 + n] = n < (int)win.size() ? win[n] : -1;
  for (int t = 0; t < VT; ++t)
    for (int n = 0; n < 16; ++n) {
      const int j = h.SegJ[t * 16 + n];
      for (int vv = 0; vv < 32; ++vv) {
        const int p_ = t * 32 + vv;
        h.W16[((size_t)t * 16 + n) * 36 + vv] = (j >= 0 && p_ < V) ? W[(size_t)order[p_] * NJ + j] : 0.f;
      }
    }
}

// =============================================================================================
// step 4: the blend basis [pose dirs | shape dirs | template] in its three images Dk / Dn / Dq, the dense skinning tiles, the permutation
// =============================================================================================
static void build_blend_basis(const float* vt, const float* sd, const float* pd, const float* W, const std::vector<int>& order, Tables& h) {
  for (int p_ = 0; p_ < VP; ++p_) h.P2V[p_] = p_ < V ? order[p_] : -1;
  for (int p_ = 0; p_ < V; ++p_) h.V2P[order[p_]] = p_;
  for (int p_ = 0; p_ < V; ++p_) {
    const int v = order[p_];                 // vertex of the file stored in row p_
    const int t = p_ >> 5, vv = p_ & 31;
    for (int c = 0; c < 3; ++c) {
      for (int k = 0; k < KF; ++k) {
        float val;
        if (k < 207) val = pd[(size_t)k * (V * 3) + v * 3 + c];
        else if (k < 217) val = sd[((size_t)v * 3 + c) * NB + (k - 207)];
        else val = vt[v * 3 + c];
        h.Dk[((((size_t)t * (KFP / 4) + (k >> 2)) * 3 + c) * 32 + vv) * 4 + (k & 3)] = val;      // K-quads [tile][k / 4][plane][32 v][4]
        h.Dn[((size_t)c * VP + p_) * KFP + k] = val;
        h.Dq[(((size_t)c * (VP / 4) + (p_ >> 2)) * KFP + k) * 4 + (p_ & 3)] = val;
      }
    }
    for (int j = 0; j < NJ; ++j) {
      h.Wjv[((size_t)t * NJ + j) * 32 + vv] = W[(size_t)v * NJ + j];
      h.Wvj[((size_t)t * 32 + vv) * 32 + j] = W[(size_t)v * NJ + j];
    }
  }
}

// =============================================================================================
// step 5: folded rest-joint regressor, in fp64: J(beta) = Jt + JS beta   (smplx vertices2joints(J_regressor, v_shaped))
// =============================================================================================
static void fold_rest_joints(const float* vt, const float* sd, const float* Jr, Tables& h) {
  for (int j = 0; j < NJ; ++j)
    for (int c = 0; c < 3; ++c) {
      double acc = 0;
      double accs[NB] = {0};
      for (int v = 0; v < V; ++v) {
        const double w = Jr[(size_t)j * V + v];
        if (w == 0.0) continue;
        acc += w * vt[v * 3 + c];
        for (int l = 0; l < NB; ++l) accs[l] += w * sd[((size_t)v * 3 + c) * NB + l];
      }
      h.Jt[j * 3 + c] = (float)acc;
      for (int l = 0; l < NB; ++l) h.JS[(j * 3 + c) * NB + l] = (float)accs[l];
    }
}

// the kinematic tree as the chain kernels walk it: parent, depth and child lists
static void set_parents(Parents& P, const int32_t* parents) {
  P.maxd = 0;
  for (int j = 0; j < NJ; ++j) {
    P.p[j] = parents[j];
    P.depth[j] = (j == 0) ? 0 : P.depth[parents[j]] + 1;
    if (P.depth[j] > P.maxd) P.maxd = P.depth[j];
  }
  int n = 0;
  for (int j = 0; j < NJ; ++j) {
    P.child_off[j] = (unsigned char)n;
    for (int q = j + 1; q < NJ; ++q)
      if (parents[q] == j) P.child[n++] = (unsigned char)q;
  }
  P.child_off[NJ] = (unsigned char)n;
  for (; n < NJ; ++n) P.child[n] = 0;
}

// =============================================================================================
// step 6: upload (into the caller's buffer or one of the library's own) and the device-side view of the tables
// =============================================================================================
static int upload_model(const std::vector<float>& h, const Tables& host, const VertexOrder& vo, const TileClasses& tc, bool bwd16,
                        const int32_t* parents, void* buffer_dev, jrr_model_t** out) {
  jrr_model* m = new jrr_model();
  void* base = buffer_dev;
  hipError_t e = hipSuccess;
  if (!base) {      // no caller buffer: the library allocates (and frees) its own
    e = hipMalloc(&base, jrr_model_bytes());
    if (e != hipSuccess) { delete m; jrr_set_error("hipMalloc(model) failed: %s", hipGetErrorString(e)); return JRR_ERR_HIP; }
  }
  e = hipMemcpy(base, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice);
  if (e != hipSuccess) { if (!buffer_dev) (void)hipFree(base); delete m; jrr_set_error("hipMemcpy(model) failed: %s", hipGetErrorString(e)); return JRR_ERR_HIP; }
  const Tables d((float*)base);
  m->base = base;
  m->owns_base = buffer_dev == nullptr;
  m->faces_area = reinterpret_cast<int*>((char*)base + round_up(MODEL_FLOATS * sizeof(float), 256));
  m->d.Dk = d.Dk; m->d.Dn = d.Dn; m->d.Dq = d.Dq; m->d.Wjv = d.Wjv; m->d.Wvj = d.Wvj; m->d.Jt = d.Jt; m->d.JS = d.JS; m->d.Wc = d.Wc;
  m->d.jl = d.Jl; m->d.tnj = d.Tnj;
  m->d.kjs = tc.kjs;
  m->d.wide_tiles = tc.wide_tiles;
  m->d.most_joints = tc.most_joints;
  for (int n = 0; n <= NJ; ++n) m->d.tile_hist[n] = tc.hist[n];
  m->d.permuted = vo.permuted ? 1 : 0;
  m->d.hint_applied = vo.hint_applied;
  m->v2p_host = nullptr;
  if (vo.permuted) { m->v2p_host = new int[V]; memcpy(m->v2p_host, host.V2P, (size_t)V * sizeof(int)); }
  m->d.p2v = vo.permuted ? d.P2V : nullptr;
  m->d.v2p = vo.permuted ? d.V2P : nullptr;
  m->d.W16 = d.W16; m->d.segid = d.SegId; m->d.segj = d.SegJ;
  m->d.bwd16 = (tc.kjs && bwd16) ? 1 : 0;
  m->d.role_kjs = (tc.kjs && !tc.wide_tiles) ? tc.kjs : 0;
  m->d.faces = nullptr;
  m->d.faces_int = nullptr;
  m->d.faces_pk = nullptr;
  m->d.faces_int_pk = nullptr;
  m->d.nfaces = 0;
  set_parents(m->d.parents, parents);
  *out = m;
  return JRR_OK;
}

extern "C" int jrr_model_create(const float* vt, const float* sd, const float* pd, const float* Jr, const float* W,
                                const int32_t* parents, jrr_model_t** out) {
  return jrr_model_create_in(vt, sd, pd, Jr, W, parents, nullptr, 0, out);
}

extern "C" int jrr_model_create_in(const float* vt, const float* sd, const float* pd, const float* Jr, const float* W,
                                   const int32_t* parents, void* buffer_dev, size_t buffer_bytes, jrr_model_t** out) {
  return jrr_model_create_hinted(vt, sd, pd, Jr, W, parents, nullptr, 0, buffer_dev, buffer_bytes, out);
}

extern "C" int jrr_model_create_hinted(const float* vt, const float* sd, const float* pd, const float* Jr, const float* W,
                                       const int32_t* parents, const int32_t* hint_vertices, int n_hint, void* buffer_dev,
                                       size_t buffer_bytes, jrr_model_t** out) {
  if (n_hint < 0 || n_hint > V || (n_hint > 0 && !hint_vertices)) { jrr_set_error("jrr_model_create_hinted: bad hint"); return JRR_ERR_ARG; }
  for (int i = 0; i < n_hint; ++i)
    if (hint_vertices[i] < 0 || hint_vertices[i] >= V) { jrr_set_error("jrr_model_create_hinted: hint vertex %d out of range", hint_vertices[i]); return JRR_ERR_ARG; }
  if (!vt || !sd || !pd || !Jr || !W || !parents || !out) { jrr_set_error("jrr_model_create: null argument"); return JRR_ERR_ARG; }
  if (buffer_dev && (buffer_bytes < jrr_model_bytes() || ((uintptr_t)buffer_dev & 255) != 0)) {
    jrr_set_error("jrr_model_create_in: the model buffer needs jrr_model_bytes() = %zu bytes, 256-byte aligned", jrr_model_bytes());
    return JRR_ERR_WORKSPACE;
  }
  for (int j = 0; j < NJ; ++j)
    if (parents[j] >= j || (j > 0 && parents[j] < 0)) { jrr_set_error("parents[%d]=%d is not a topologically ordered tree", j, parents[j]); return JRR_ERR_ARG; }
  const Knobs kn = read_knobs();      // as the environment is NOW: one process may create variant models
  std::vector<float> h(MODEL_FLOATS, 0.f);
  Tables host(h.data());
  const VertexOrder vo = choose_vertex_order(W, parents, hint_vertices, n_hint, kn.vertex_order_sorted);
  const TileClasses tc = classify_tiles(W, vo.order, kn);
  if (tc.kjs) {
    build_tile_lists(W, vo.order, tc, host);
    build_backward_windows(W, vo.order, tc.lists, host);
  }
  build_blend_basis(vt, sd, pd, W, vo.order, host);
  fold_rest_joints(vt, sd, Jr, host);
  return upload_model(h, host, vo, tc, kn.bwd16, parents, buffer_dev, out);
}

extern "C" int jrr_model_set_faces(jrr_model_t* m, const int32_t* faces, int n_faces) {
  if (!m || !faces || n_faces <= 0) return JRR_ERR_ARG;
  if (n_faces > MAX_FACES) { jrr_set_error("%d faces: the rasteriser holds at most %d", n_faces, MAX_FACES); return JRR_ERR_ARG; }
  for (int i = 0; i < n_faces * 3; ++i)
    if (faces[i] < 0 || faces[i] >= V) { jrr_set_error("face index %d out of range", faces[i]); return JRR_ERR_ARG; }
  // both index lists live in the tail of the model buffer (jrr_model_bytes): no allocation here
  m->d.faces = m->faces_area;
  m->d.faces_int = nullptr;
  JRR_HIP(hipMemcpy(m->d.faces, faces, (size_t)n_faces * 3 * sizeof(int), hipMemcpyHostToDevice));
  if (m->v2p_host) {      // the fused rasteriser reads the vertices in the internal order: faces in row indices
    std::vector<int32_t> fi((size_t)n_faces * 3);
    for (size_t i = 0; i < fi.size(); ++i) fi[i] = m->v2p_host[faces[i]];
    m->d.faces_int = m->faces_area + (size_t)MAX_FACES * 3;
    JRR_HIP(hipMemcpy(m->d.faces_int, fi.data(), fi.size() * sizeof(int), hipMemcpyHostToDevice));
  }
  // the rasteriser reads a face as ONE 8-byte record (three 13-bit vertex indices): one gather per face where three strided
  // 4-byte ones were the resolve pass's bound
  auto pack = [&](const int32_t* f3, unsigned* dst) -> int {
    std::vector<unsigned> pk((size_t)n_faces * 2);
    for (int i = 0; i < n_faces; ++i) { pk[2 * i] = (unsigned)f3[3 * i] | ((unsigned)f3[3 * i + 1] << 13); pk[2 * i + 1] = (unsigned)f3[3 * i + 2]; }
    return hipMemcpy(dst, pk.data(), pk.size() * sizeof(unsigned), hipMemcpyHostToDevice) == hipSuccess ? 0 : 1;
  };
  static_assert(V <= 8192, "packed face records hold 13-bit vertex indices");
  m->d.faces_pk = reinterpret_cast<unsigned*>(m->faces_area + (size_t)2 * MAX_FACES * 3);
  m->d.faces_int_pk = nullptr;
  if (pack(faces, m->d.faces_pk)) { jrr_set_error("hipMemcpy(faces) failed"); return JRR_ERR_HIP; }
  if (m->v2p_host) {
    std::vector<int32_t> fi((size_t)n_faces * 3);
    for (size_t i = 0; i < fi.size(); ++i) fi[i] = m->v2p_host[faces[i]];
    m->d.faces_int_pk = m->d.faces_pk + (size_t)MAX_FACES * 2;
    if (pack(fi.data(), m->d.faces_int_pk)) { jrr_set_error("hipMemcpy(faces) failed"); return JRR_ERR_HIP; }
  }
  m->d.nfaces = n_faces;
  return JRR_OK;
}

extern "C" void jrr_model_destroy(jrr_model_t* m) {
  if (!m) return;
  if (m->base && m->owns_base) (void)hipFree(m->base);
  delete[] m->v2p_host;
  delete m;
}

extern "C" int jrr_model_info(const jrr_model_t* m, int32_t* out, int n) {
  if (!m || !out) return JRR_ERR_ARG;
  int32_t v[4 + NJ + 2] = {m->d.kjs, m->d.wide_tiles, m->d.most_joints, m->d.permuted};
  for (int k = 0; k <= NJ; ++k) v[4 + k] = m->d.tile_hist[k];
  v[4 + NJ + 1] = m->d.hint_applied;
  for (int i = 0; i < n && i < 4 + NJ + 2; ++i) out[i] = v[i];
  return JRR_OK;
}
