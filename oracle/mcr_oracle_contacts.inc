// oracle/mcr_oracle_contacts.inc — TEST INFRASTRUCTURE (included by mcr_oracle.cpp)
//
// Car<->car rigid contacts and the island solve: restates the published algorithms of
// Box2D 2.3.x  b2CollidePolygons / b2ClipSegmentToLine / b2WorldManifold / b2ContactSolver
// (velocity + block solver + position) and b2Island::Solve / b2World::Solve.
//
// Orderings that real Box2D derives from its broadphase proxy ids and intrusive lists (not
// reproducible without the library) are DEFINED here and mirrored by the product:
//   * fixture pair (A,B): A = lower (car, fixture) where fixture 0..3 = hull polys, 4..7 = wheels
//   * contact order: ascending (carA, fixA, carB, fixB)
//   * joint order inside a car: 3,2,1,0 (island DFS order from the newest body — see DESIGN.md)
//
// The product's manifold store holds MCR_CC_MAX records per env.  orc_set_contact_cap(h, cap) mirrors that (DESIGN.md §3.1, THE DROP RULE):
// of the touching fixture pairs of a step, found at the poses entering it, the first `cap` are kept in the order k_collide finds them —
// pairs of cars ascending by (a, b), a < b; within a pair of cars ascending by fixture-of-a * 8 + fixture-of-b — whichever of the two
// fixtures is fixtureA.  The others are dropped for that step: no constraint, no island link, no warm start from them next step.
// The kept set is a function of the entry poses alone.  cap 0 (the default): no cap, Box2D's behaviour.
namespace {

// what the contact code reached, per env (orc_contact_coverage; Env::cov).  MAX rows hold a maximum, the others count.
enum { COV_MAX_MANIFOLDS = 0, COV_BLOCK_BOTH, COV_BLOCK_X1, COV_BLOCK_X2, COV_BLOCK_NEITHER, COV_BLOCK_NONE, COV_ILL_CONDITIONED, COV_FACE_A, COV_FACE_B,
       COV_FLIPPED, COV_POS_SWEEPS_ALL, COV_ID_MATCH, COV_ID_MISS, COV_TRANSLATION_CLAMP, COV_ROTATION_CLAMP, COV_MAX_ISLAND_CARS, COV_MAX_CANDIDATES,
       COV_DROPPED, COV_ILL_THEN_WELL, COV_ROWS };
static_assert((int)COV_ROWS <= (int)ORC_COV_ROWS, "Env::cov is too small");
inline void cov_max(Env& E, int row, long long v) { if (v > E.cov[row]) E.cov[row] = v; }

struct CPoint { V2 local; f32 nImp, tImp; uint32_t id; };
struct CManifold { int type; V2 localNormal, localPoint; int n; CPoint p[2]; };
struct CarContact {
  int carA, fixA, carB, fixB;
  CManifold m;
  bool ill = false, prev_ill = false;   // this step / the pair's last step solved a two-point manifold as one point (ill-conditioned K)
  int found;                     // where k_collide finds the pair: (a * 8 + b) * 64 + fixture of a * 8 + fixture of b, a < b
};
struct ContactStore {
  std::vector<CarContact> cur;   // touching contacts of the current step, defined order
  std::vector<CarContact> prev;  // previous step (warm-start matching by feature id)
  std::vector<int> cord;         // the order the last step solved `cur` in
  int jord[8][4];                // ... and each car's joints
  int candidates = 0;            // touching pairs of the last step before the cap
};
ContactStore& store_of(Env& E) {
  if (!E.contact_store) E.contact_store = new ContactStore();
  return *(ContactStore*)E.contact_store;
}
void contacts_free(Env& E) { delete (ContactStore*)E.contact_store; E.contact_store = nullptr; }
void contacts_reset(Env& E) { ContactStore& S = store_of(E); S.cur.clear(); S.prev.clear(); S.cord.clear(); S.candidates = 0; }

inline const Poly& fixture_poly(const Env& E, int fix) { return fix < 4 ? E.S.hull[fix] : E.S.wheel; }
inline int fixture_body(int fix) { return fix < 4 ? 0 : fix - 3; }

struct ClipV { V2 v; uint32_t id; };
inline uint32_t mkid(int ia, int ib, int ta, int tb) { return (uint32_t)(ia & 255) | ((uint32_t)(ib & 255) << 8) | ((uint32_t)ta << 16) | ((uint32_t)tb << 24); }
inline uint32_t flipid(uint32_t id) { return ((id >> 8) & 255) | ((id & 255) << 8) | (((id >> 24) & 255) << 16) | (((id >> 16) & 255) << 24); }
inline Xf mulT(const Xf& A, const Xf& B) {   // b2MulT(A,B) = A^-1 * B
  Xf C; C.q.s = A.q.c * B.q.s - A.q.s * B.q.c; C.q.c = A.q.c * B.q.c + A.q.s * B.q.s;
  C.p = mulT(A.q, B.p - A.p); return C;
}
inline V2 mulT(const Xf& T, V2 v) { f32 px = v.x - T.p.x, py = v.y - T.p.y; return v2(T.q.c * px + T.q.s * py, -T.q.s * px + T.q.c * py); }

f32 find_max_separation(int* edge, const Poly& p1, const Xf& xf1, const Poly& p2, const Xf& xf2) {
  Xf xf = mulT(xf2, xf1);
  int best = 0; f32 maxSep = -3.402823466e+38f;
  for (int i = 0; i < p1.n; ++i) {
    V2 n = mul(xf.q, p1.nrm[i]);
    V2 v1 = mul(xf, p1.v[i]);
    f32 si = 3.402823466e+38f;
    for (int j = 0; j < p2.n; ++j) { f32 sij = dot(n, p2.v[j] - v1); if (sij < si) si = sij; }
    if (si > maxSep) { maxSep = si; best = i; }
  }
  *edge = best; return maxSep;
}
int clip_segment(ClipV out[2], const ClipV in[2], V2 normal, f32 offset, int vertexIndexA) {
  int n = 0;
  f32 d0 = dot(normal, in[0].v) - offset, d1 = dot(normal, in[1].v) - offset;
  if (d0 <= 0.0f) out[n++] = in[0];
  if (d1 <= 0.0f) out[n++] = in[1];
  if (d0 * d1 < 0.0f) {
    f32 interp = d0 / (d0 - d1);
    out[n].v = in[0].v + interp * (in[1].v - in[0].v);
    out[n].id = mkid(vertexIndexA, (in[0].id >> 8) & 255, 0 /*vertex*/, 1 /*face*/);
    ++n;
  }
  return n;
}
void collide_polygons(CManifold& M, const Poly& pA, const Xf& xfA, const Poly& pB, const Xf& xfB) {
  M.n = 0;
  const f32 totalRadius = b2_polygonRadius + b2_polygonRadius;
  int edgeA = 0; f32 sepA = find_max_separation(&edgeA, pA, xfA, pB, xfB);
  if (sepA > totalRadius) return;
  int edgeB = 0; f32 sepB = find_max_separation(&edgeB, pB, xfB, pA, xfA);
  if (sepB > totalRadius) return;
  const Poly *p1, *p2; Xf xf1, xf2; int edge1; int flip;
  const f32 k_tol = 0.1f * b2_linearSlop;
  if (sepB > sepA + k_tol) { p1 = &pB; p2 = &pA; xf1 = xfB; xf2 = xfA; edge1 = edgeB; M.type = 2; flip = 1; }
  else { p1 = &pA; p2 = &pB; xf1 = xfA; xf2 = xfB; edge1 = edgeA; M.type = 1; flip = 0; }
  // incident edge
  ClipV inc[2];
  {
    V2 normal1 = mulT(xf2.q, mul(xf1.q, p1->nrm[edge1]));
    int index = 0; f32 minDot = 3.402823466e+38f;
    for (int i = 0; i < p2->n; ++i) { f32 d = dot(normal1, p2->nrm[i]); if (d < minDot) { minDot = d; index = i; } }
    int i1 = index, i2 = i1 + 1 < p2->n ? i1 + 1 : 0;
    inc[0].v = mul(xf2, p2->v[i1]); inc[0].id = mkid(edge1, i1, 1, 0);
    inc[1].v = mul(xf2, p2->v[i2]); inc[1].id = mkid(edge1, i2, 1, 0);
  }
  int iv1 = edge1, iv2 = edge1 + 1 < p1->n ? edge1 + 1 : 0;
  V2 v11 = p1->v[iv1], v12 = p1->v[iv2];
  V2 localTangent = v12 - v11;
  { f32 len = length(localTangent); if (len >= b2_epsilon) { f32 inv = 1.0f / len; localTangent.x *= inv; localTangent.y *= inv; } }
  V2 localNormal = cross(localTangent, 1.0f);
  V2 planePoint = 0.5f * (v11 + v12);
  V2 tangent = mul(xf1.q, localTangent);
  V2 normal = cross(tangent, 1.0f);
  v11 = mul(xf1, v11); v12 = mul(xf1, v12);
  f32 frontOffset = dot(normal, v11);
  f32 sideOffset1 = -dot(tangent, v11) + totalRadius;
  f32 sideOffset2 = dot(tangent, v12) + totalRadius;
  ClipV c1[2], c2[2];
  if (clip_segment(c1, inc, -tangent, sideOffset1, iv1) < 2) return;
  if (clip_segment(c2, c1, tangent, sideOffset2, iv2) < 2) return;
  M.localNormal = localNormal; M.localPoint = planePoint;
  int pc = 0;
  for (int i = 0; i < 2; ++i) {
    f32 separation = dot(normal, c2[i].v) - frontOffset;
    if (separation <= totalRadius) {
      CPoint& cp = M.p[pc];
      cp.local = mulT(xf2, c2[i].v);
      cp.id = flip ? flipid(c2[i].id) : c2[i].id;
      cp.nImp = cp.tImp = 0.0f;
      ++pc;
    }
  }
  M.n = pc;
}

bool car_fixture_id_lower(const Env& E, int pf, int pg);   // mcr_oracle.cpp: proxy id of car fixture pf < that of pg (world mode 1; false in a fresh world for pf > pg)
// b2ContactManager::Collide for the dynamic (car<->car) pairs at the poses entering the step.
void collide_cars(Env& E) {
  ContactStore& S = store_of(E);
  S.prev.swap(S.cur); S.cur.clear(); S.cord.clear(); S.candidates = 0;
  if (!E.enable_car_contacts) return;
  const int N = E.N;
  {   // b2ContactManager::Collide destroys the contacts whose fat AABBs ceased to overlap
    const int F = N * 8;
    size_t w = 0;
    for (size_t i = 0; i < E.ccl.size(); ++i) {
      const auto pr = E.ccl[i];
      const AABB& fa = E.fix_fat[pr.first]; const AABB& fb = E.fix_fat[pr.second];
      const bool overlap = !(fb.lo.x - fa.hi.x > 0.0f || fb.lo.y - fa.hi.y > 0.0f || fa.lo.x - fb.hi.x > 0.0f || fa.lo.y - fb.hi.y > 0.0f);     // b2TestOverlap(b2AABB, b2AABB)
      if (overlap) E.ccl[w++] = pr; else E.cc_exists[(size_t)pr.first * F + pr.second] = 0;
    }
    E.ccl.resize(w);
  }
  // tight fixture AABBs (+radius) for a cheap reject; the manifold routine is the arbiter.
  std::vector<V2> lo(N * 8), hi(N * 8);
  for (int c = 0; c < N; ++c) for (int f = 0; f < 8; ++f) {
    const Poly& P = fixture_poly(E, f); const Xf& xf = E.cars[c].b[fixture_body(f)].xf;
    V2 l = v2(3.4e38f, 3.4e38f), h = v2(-3.4e38f, -3.4e38f);
    for (int i = 0; i < P.n; ++i) { V2 p = mul(xf, P.v[i]); l.x = std::min(l.x, p.x); l.y = std::min(l.y, p.y); h.x = std::max(h.x, p.x); h.y = std::max(h.y, p.y); }
    lo[c * 8 + f] = v2(l.x - 0.05f, l.y - 0.05f); hi[c * 8 + f] = v2(h.x + 0.05f, h.y + 0.05f);
  }
  for (int a = 0; a < N; ++a) for (int fa = 0; fa < 8; ++fa) for (int b = a + 1; b < N; ++b) for (int fb = 0; fb < 8; ++fb) {
    if (fa >= 4 && fb >= 4) continue;                 // wheel(0x20,mask 1) vs wheel: filtered
    int ia = a * 8 + fa, ib = b * 8 + fb;
    if (lo[ia].x > hi[ib].x || hi[ia].x < lo[ib].x || lo[ia].y > hi[ib].y || hi[ia].y < lo[ib].y) continue;
    // fixtureA of a contact = the fixture with the LOWER proxy id (b2BroadPhase::UpdatePairs hands AddPair (min, max), b2Contact::Create keeps
    // the order for polygon pairs): car a's in a fresh world; whichever the tree's free list gave the lower id in a world that lives on
    const bool flip = car_fixture_id_lower(E, ib, ia);
    CarContact C; C.found = (a * 8 + b) * 64 + fa * 8 + fb;
    if (!flip) { C.carA = a; C.fixA = fa; C.carB = b; C.fixB = fb; } else { C.carA = b; C.fixA = fb; C.carB = a; C.fixB = fa; }
    collide_polygons(C.m, fixture_poly(E, C.fixA), E.cars[C.carA].b[fixture_body(C.fixA)].xf, fixture_poly(E, C.fixB), E.cars[C.carB].b[fixture_body(C.fixB)].xf);
    if (C.m.n == 0) continue;
    S.cur.push_back(C);
  }
  S.candidates = (int)S.cur.size();
  cov_max(E, COV_MAX_CANDIDATES, S.candidates);
  if (E.contact_cap > 0 && (int)S.cur.size() > E.contact_cap) {     // THE DROP RULE (header): the first `cap` in the order k_collide finds them
    std::vector<int> key; for (const CarContact& C : S.cur) key.push_back(C.found);
    std::sort(key.begin(), key.end());
    const int last = key[E.contact_cap - 1];
    size_t w = 0;
    for (size_t i = 0; i < S.cur.size(); ++i) if (S.cur[i].found <= last) S.cur[w++] = S.cur[i];
    E.cov[COV_DROPPED] += (long long)(S.cur.size() - w);
    S.cur.resize(w);
  }
  for (CarContact& C : S.cur) {
    E.cov[C.m.type == 1 ? COV_FACE_A : COV_FACE_B] += 1;
    if (C.carA > C.carB) E.cov[COV_FLIPPED] += 1;
    for (const CarContact& O : S.prev)               // b2Contact::Update id matching
      if (O.carA == C.carA && O.fixA == C.fixA && O.carB == C.carB && O.fixB == C.fixB) {
        C.prev_ill = O.ill;
        for (int i = 0; i < C.m.n; ++i) {
          bool hit = false;
          for (int j = 0; j < O.m.n; ++j)
            if (O.m.p[j].id == C.m.p[i].id) { C.m.p[i].nImp = O.m.p[j].nImp; C.m.p[i].tImp = O.m.p[j].tImp; hit = true; break; }
          E.cov[hit ? COV_ID_MATCH : COV_ID_MISS] += 1;
        }
      }
  }
  cov_max(E, COV_MAX_MANIFOLDS, (long long)S.cur.size());
}

struct VCPoint { V2 rA, rB; f32 nImp, tImp, normalMass, tangentMass, velocityBias; };
struct VC {
  VCPoint p[2]; V2 normal; f32 k11, k12, k21, k22; f32 nm11, nm12, nm21, nm22; int n;
  Body *A, *B; f32 friction;
};

void world_manifold(const CManifold& M, const Xf& xfA, const Xf& xfB, V2* normal, V2 pts[2]) {
  const f32 rA = b2_polygonRadius, rB = b2_polygonRadius;
  if (M.type == 1) {
    *normal = mul(xfA.q, M.localNormal);
    V2 planePoint = mul(xfA, M.localPoint);
    for (int i = 0; i < M.n; ++i) {
      V2 clip = mul(xfB, M.p[i].local);
      V2 cA = clip + (rA - dot(clip - planePoint, *normal)) * (*normal);
      V2 cB = clip - rB * (*normal);
      pts[i] = 0.5f * (cA + cB);
    }
  } else {
    *normal = mul(xfB.q, M.localNormal);
    V2 planePoint = mul(xfB, M.localPoint);
    for (int i = 0; i < M.n; ++i) {
      V2 clip = mul(xfA, M.p[i].local);
      V2 cB = clip + (rB - dot(clip - planePoint, *normal)) * (*normal);
      V2 cA = clip - rA * (*normal);
      pts[i] = 0.5f * (cA + cB);
    }
    *normal = -(*normal);
  }
}

void contact_solve_velocity(VC& c, long long* cov) {
  Body& A = *c.A; Body& B = *c.B;
  f32 mA = A.invMass, iA = A.invI, mB = B.invMass, iB = B.invI;
  V2 vA = A.v, vB = B.v; f32 wA = A.w, wB = B.w;
  V2 normal = c.normal; V2 tangent = cross(normal, 1.0f);
  for (int j = 0; j < c.n; ++j) {
    VCPoint& p = c.p[j];
    V2 dv = vB + cross(wB, p.rB) - vA - cross(wA, p.rA);
    f32 vt = dot(dv, tangent) - 0.0f;
    f32 lambda = p.tangentMass * (-vt);
    f32 maxF = c.friction * p.nImp;
    f32 newImp = clampf(p.tImp + lambda, -maxF, maxF);
    lambda = newImp - p.tImp; p.tImp = newImp;
    V2 P = lambda * tangent;
    vA = vA - mA * P; wA -= iA * cross(p.rA, P);
    vB = vB + mB * P; wB += iB * cross(p.rB, P);
  }
  if (c.n == 1) {
    VCPoint& p = c.p[0];
    V2 dv = vB + cross(wB, p.rB) - vA - cross(wA, p.rA);
    f32 vn = dot(dv, normal);
    f32 lambda = -p.normalMass * (vn - p.velocityBias);
    f32 newImp = std::max(p.nImp + lambda, 0.0f);
    lambda = newImp - p.nImp; p.nImp = newImp;
    V2 P = lambda * normal;
    vA = vA - mA * P; wA -= iA * cross(p.rA, P);
    vB = vB + mB * P; wB += iB * cross(p.rB, P);
  } else {
    VCPoint& cp1 = c.p[0]; VCPoint& cp2 = c.p[1];
    V2 a = v2(cp1.nImp, cp2.nImp);
    V2 dv1 = vB + cross(wB, cp1.rB) - vA - cross(wA, cp1.rA);
    V2 dv2 = vB + cross(wB, cp2.rB) - vA - cross(wA, cp2.rA);
    f32 vn1 = dot(dv1, normal), vn2 = dot(dv2, normal);
    V2 b = v2(vn1 - cp1.velocityBias, vn2 - cp2.velocityBias);
    b = b - v2(c.k11 * a.x + c.k12 * a.y, c.k21 * a.x + c.k22 * a.y);
    V2 x; bool ok = false;
    for (;;) {
      x = -v2(c.nm11 * b.x + c.nm12 * b.y, c.nm21 * b.x + c.nm22 * b.y);
      if (x.x >= 0.0f && x.y >= 0.0f) { ok = true; cov[COV_BLOCK_BOTH] += 1; break; }
      x.x = -cp1.normalMass * b.x; x.y = 0.0f; vn1 = 0.0f; vn2 = c.k21 * x.x + b.y;
      if (x.x >= 0.0f && vn2 >= 0.0f) { ok = true; cov[COV_BLOCK_X1] += 1; break; }
      x.x = 0.0f; x.y = -cp2.normalMass * b.y; vn1 = c.k12 * x.y + b.x; vn2 = 0.0f;
      if (x.y >= 0.0f && vn1 >= 0.0f) { ok = true; cov[COV_BLOCK_X2] += 1; break; }
      x.x = 0.0f; x.y = 0.0f; vn1 = b.x; vn2 = b.y;
      if (vn1 >= 0.0f && vn2 >= 0.0f) { ok = true; cov[COV_BLOCK_NEITHER] += 1; break; }
      cov[COV_BLOCK_NONE] += 1;
      break;
    }
    if (ok) {
      V2 d = x - a;
      V2 P1 = d.x * normal, P2 = d.y * normal;
      vA = vA - mA * (P1 + P2); wA -= iA * (cross(cp1.rA, P1) + cross(cp2.rA, P2));
      vB = vB + mB * (P1 + P2); wB += iB * (cross(cp1.rB, P1) + cross(cp2.rB, P2));
      cp1.nImp = x.x; cp2.nImp = x.y;
    }
  }
  A.v = vA; A.w = wA; B.v = vB; B.w = wB;
}

// returns min separation over the contact's points
f32 contact_solve_position(const CarContact& C, Body& A, Body& B) {
  f32 mA = A.invMass, iA = A.invI, mB = B.invMass, iB = B.invI;
  V2 cA = A.c, cB = B.c; f32 aA = A.a, aB = B.a;
  f32 minSep = 0.0f;
  for (int j = 0; j < C.m.n; ++j) {
    Xf xfA, xfB; xfA.q.Set(aA); xfB.q.Set(aB);
    xfA.p = cA - mul(xfA.q, A.lc); xfB.p = cB - mul(xfB.q, B.lc);
    V2 normal, point; f32 separation;
    if (C.m.type == 1) {
      normal = mul(xfA.q, C.m.localNormal);
      V2 planePoint = mul(xfA, C.m.localPoint);
      V2 clip = mul(xfB, C.m.p[j].local);
      separation = dot(clip - planePoint, normal) - b2_polygonRadius - b2_polygonRadius;
      point = clip;
    } else {
      normal = mul(xfB.q, C.m.localNormal);
      V2 planePoint = mul(xfB, C.m.localPoint);
      V2 clip = mul(xfA, C.m.p[j].local);
      separation = dot(clip - planePoint, normal) - b2_polygonRadius - b2_polygonRadius;
      point = clip;
      normal = -normal;
    }
    V2 rA = point - cA, rB = point - cB;
    minSep = std::min(minSep, separation);
    f32 Cc = clampf(b2_baumgarte * (separation + b2_linearSlop), -b2_maxLinearCorrection, 0.0f);
    f32 rnA = cross(rA, normal), rnB = cross(rB, normal);
    f32 K = mA + mB + iA * rnA * rnA + iB * rnB * rnB;
    f32 impulse = K > 0.0f ? -Cc / K : 0.0f;
    V2 P = impulse * normal;
    cA = cA - mA * P; aA -= iA * cross(rA, P);
    cB = cB + mB * P; aB += iB * cross(rB, P);
  }
  A.c = cA; A.a = aA; B.c = cB; B.a = aB;
  return minSep;
}

const int JOINT_ORDER[4] = {3, 2, 1, 0};

// b2World::Solve's island construction for the cars (island order 1): seeds from m_bodyList (head = the body created LAST: car N-1's
// wheel 3, 2, 1, 0, its hull, car N-2's ..); a depth-first search with an explicit stack that, for the body it pops, appends the
// touching contacts of the body's contact-edge list (head = the contact created last) and then the joints of its joint-edge list
// (hull: j3, j2, j1, j0 — created in wheel order, inserted at the head; a wheel: its one joint), pushing the other bodies.
// b2Island::Solve then runs the joints and the contacts in the order they were appended.  Constraints of different islands — and the
// joints of different cars — touch disjoint bodies and commute, so the result is: per car an order of its 4 joints, and one order of
// the touching contacts.
void island_dfs(Env& E, const ContactStore& S, int (*jord)[4], std::vector<int>& cord) {
  const int N = E.N, F = N * 8;
  std::vector<int> cur_of((size_t)F * F, -1);                              // fixture pair -> index in S.cur (touching contacts only)
  for (size_t i = 0; i < S.cur.size(); ++i) { const int ka = S.cur[i].carA * 8 + S.cur[i].fixA, kb = S.cur[i].carB * 8 + S.cur[i].fixB; cur_of[(size_t)std::min(ka, kb) * F + std::max(ka, kb)] = (int)i; }
  std::vector<uint8_t> bflag(N * 5, 0), cflag(S.cur.size(), 0), jflag(N * 4, 0);
  std::vector<int> jn(N, 0), stack;
  cord.clear();
  auto body_of = [](int pf) { return (pf / 8) * 5 + fixture_body(pf & 7); };
  for (int c = N - 1; c >= 0; --c) for (int k = 4; k >= 0; --k) {
    const int seed = c * 5 + k;
    if (bflag[seed]) continue;
    stack.clear(); stack.push_back(seed); bflag[seed] = 1;
    while (!stack.empty()) {
      const int b = stack.back(); stack.pop_back();
      const int bc = b / 5, bk = b % 5;
      for (int i = (int)E.ccl.size() - 1; i >= 0; --i) {                    // contact edges, newest first
        const int pa = E.ccl[i].first, pb = E.ccl[i].second;
        const int ba = body_of(pa), bb = body_of(pb);
        if (ba != b && bb != b) continue;
        // S.cur names a pair (lower (car, fixture) first); the broadphase pair is (lower proxy id first): the same in a fresh world
        const int lo = std::min(pa, pb), hi = std::max(pa, pb);
        const int ci = cur_of[(size_t)lo * F + hi];
        if (ci < 0 || cflag[ci]) continue;                                  // not touching / already in the island
        cord.push_back(ci); cflag[ci] = 1;
        const int other = ba == b ? bb : ba;
        if (!bflag[other]) { stack.push_back(other); bflag[other] = 1; }
      }
      if (bk == 0) {
        for (int q = 3; q >= 0; --q) if (!jflag[bc * 4 + q]) { jord[bc][jn[bc]++] = q; jflag[bc * 4 + q] = 1; const int w = bc * 5 + q + 1; if (!bflag[w]) { stack.push_back(w); bflag[w] = 1; } }
      } else {
        const int q = bk - 1;
        if (!jflag[bc * 4 + q]) { jord[bc][jn[bc]++] = q; jflag[bc * 4 + q] = 1; const int hb = bc * 5; if (!bflag[hb]) { stack.push_back(hb); bflag[hb] = 1; } }
      }
    }
  }
}

// b2World::Solve + b2Island::Solve restricted to cars (tiles are static sensors: no island links).
void world_solve(Env& E, f32 h, int velIters, int posIters) {
  const int N = E.N;
  E.dbg_pos_iters = 0;
  collide_cars(E);
  ContactStore& S = store_of(E);
  // islands: union-find over cars linked by touching contacts
  std::vector<int> isl(N); for (int c = 0; c < N; ++c) isl[c] = c;
  auto find = [&](int x) { while (isl[x] != x) x = isl[x]; return x; };
  for (const CarContact& C : S.cur) { int a = find(C.carA), b = find(C.carB); if (a != b) isl[std::max(a, b)] = std::min(a, b); }
  for (int c = 0; c < N; ++c) isl[c] = find(c);
  for (int r = 0; r < N; ++r) { int n = 0; for (int c = 0; c < N; ++c) n += isl[c] == r; if (n > 1) cov_max(E, COV_MAX_ISLAND_CARS, n); }
  // the order of joints (per car) and contacts: DEFINED (island order 0, what the kernels implement) or Box2D's island DFS (1)
  int (&jord)[8][4] = S.jord; std::vector<int>& cord = S.cord; cord.resize(S.cur.size());
  for (int c = 0; c < 8; ++c) for (int q = 0; q < 4; ++q) jord[c][q] = 0;
  for (int c = 0; c < N; ++c) for (int q = 0; q < 4; ++q) jord[c][q] = JOINT_ORDER[q];
  for (size_t i = 0; i < S.cur.size(); ++i) cord[i] = (int)i;
  if (E.island_order >= 1) island_dfs(E, S, jord, cord);
  if (E.island_order == 2) for (int c = 0; c < N; ++c) for (int q = 0; q < 4; ++q) jord[c][q] = JOINT_ORDER[q];     // (stage 1 of the kernels: the contact order only)
  E.dbg_island_diff = 0;
  for (int c = 0; c < N; ++c) for (int q = 0; q < 4; ++q) if (jord[c][q] != JOINT_ORDER[q]) E.dbg_island_diff |= 1;     // a car entered through a wheel other than 3
  for (size_t i = 0; i < cord.size(); ++i) if (cord[i] != (int)i) E.dbg_island_diff |= 2;                              // contacts not in ascending (carA, fixA, carB, fixB)

  // integrate velocities
  for (int c = 0; c < N; ++c) for (int k = 0; k < 5; ++k) {
    Body& b = E.cars[c].b[k];
    b.v = b.v + h * (b.invMass * b.force);
    b.w += h * b.invI * 0.0f;
  }
  // contact velocity constraints + warm start
  std::vector<VC> vcs(S.cur.size());
  for (size_t i = 0; i < S.cur.size(); ++i) {
    const CarContact& C = S.cur[i]; VC& vc = vcs[i];
    Body& A = E.cars[C.carA].b[fixture_body(C.fixA)]; Body& B = E.cars[C.carB].b[fixture_body(C.fixB)];
    vc.A = &A; vc.B = &B; vc.n = C.m.n; vc.friction = sqrtf(0.2f * 0.2f);
    f32 mA = A.invMass, iA = A.invI, mB = B.invMass, iB = B.invI;
    Xf xfA, xfB; xfA.q.Set(A.a); xfB.q.Set(B.a);
    xfA.p = A.c - mul(xfA.q, A.lc); xfB.p = B.c - mul(xfB.q, B.lc);
    V2 pts[2]; world_manifold(C.m, xfA, xfB, &vc.normal, pts);
    for (int j = 0; j < vc.n; ++j) {
      VCPoint& p = vc.p[j];
      p.nImp = 1.0f * C.m.p[j].nImp; p.tImp = 1.0f * C.m.p[j].tImp;
      p.rA = pts[j] - A.c; p.rB = pts[j] - B.c;
      f32 rnA = cross(p.rA, vc.normal), rnB = cross(p.rB, vc.normal);
      f32 kN = mA + mB + iA * rnA * rnA + iB * rnB * rnB;
      p.normalMass = kN > 0.0f ? 1.0f / kN : 0.0f;
      V2 tangent = cross(vc.normal, 1.0f);
      f32 rtA = cross(p.rA, tangent), rtB = cross(p.rB, tangent);
      f32 kT = mA + mB + iA * rtA * rtA + iB * rtB * rtB;
      p.tangentMass = kT > 0.0f ? 1.0f / kT : 0.0f;
      p.velocityBias = 0.0f;                                 // restitution 0
    }
    if (vc.n == 2) {
      f32 rn1A = cross(vc.p[0].rA, vc.normal), rn1B = cross(vc.p[0].rB, vc.normal);
      f32 rn2A = cross(vc.p[1].rA, vc.normal), rn2B = cross(vc.p[1].rB, vc.normal);
      f32 k11 = mA + mB + iA * rn1A * rn1A + iB * rn1B * rn1B;
      f32 k22 = mA + mB + iA * rn2A * rn2A + iB * rn2B * rn2B;
      f32 k12 = mA + mB + iA * rn1A * rn2A + iB * rn1B * rn2B;
      if (k11 * k11 < 1000.0f * (k11 * k22 - k12 * k12)) {
        vc.k11 = k11; vc.k12 = k12; vc.k21 = k12; vc.k22 = k22;
        f32 det = k11 * k22 - k12 * k12; if (det != 0.0f) det = 1.0f / det;
        vc.nm11 = det * k22; vc.nm12 = -det * k12; vc.nm21 = -det * k12; vc.nm22 = det * k11;
        if (C.prev_ill) E.cov[COV_ILL_THEN_WELL] += 1;      // (the second point's stored impulse is the one the fallback left alone)
      } else { vc.n = 1; S.cur[i].ill = true; E.cov[COV_ILL_CONDITIONED] += 1; }
    }
  }
  for (int oi : cord) {   // WarmStart
    VC& vc = vcs[oi];
    Body& A = *vc.A; Body& B = *vc.B;
    V2 tangent = cross(vc.normal, 1.0f);
    for (int j = 0; j < vc.n; ++j) {
      V2 P = vc.p[j].nImp * vc.normal + vc.p[j].tImp * tangent;
      A.w -= A.invI * cross(vc.p[j].rA, P); A.v = A.v - A.invMass * P;
      B.w += B.invI * cross(vc.p[j].rB, P); B.v = B.v + B.invMass * P;
    }
  }
  for (int c = 0; c < N; ++c) for (int q = 0; q < 4; ++q) joint_init(E.cars[c], jord[c][q]);
  for (int c = 0; c < N; ++c) for (int q = 0; q < 4; ++q) {      // orc_dynamics_coverage: the limit states the velocity sweeps run with
    const int ls = E.cars[c].j[q].limitState; long long* dy = E.dyn_last(c);
    dy[DY_LIM_J0 + q] = ls; dy[DY_LIM_INACTIVE + ls] += 1;
  }
  // diagnostics (orc_debug_fixed_point): the sweep is a pure function of (velocities, accumulated impulses) — masses, anchors, motor speeds
  // and limit states are constants of the step —, so once a sweep changes none of them no later sweep does.  Per car without contacts:
  // the first sweep that is the identity (velIters: none was).
  struct Snap { f32 v[15]; f32 imp[16]; };
  auto snap_of = [](const Car& car) { Snap s; for (int k = 0; k < 5; ++k) { s.v[3 * k] = car.b[k].v.x; s.v[3 * k + 1] = car.b[k].v.y; s.v[3 * k + 2] = car.b[k].w; }
    for (int q = 0; q < 4; ++q) { s.imp[4 * q] = car.j[q].impulse.x; s.imp[4 * q + 1] = car.j[q].impulse.y; s.imp[4 * q + 2] = car.j[q].impulse.z; s.imp[4 * q + 3] = car.j[q].motorImpulse; } return s; };
  const bool track_fix = E.dbg_fixed_point != nullptr && vcs.empty();
  std::vector<int> fix_at(N, velIters);
  // diagnostics (orc_debug_cycle): the first sweep after which the env's whole iteration state (all cars + the contacts' accumulated impulses)
  // equals the state 1..8 sweeps earlier — from there on the sweeps repeat with that period
  const bool track_cyc = E.dbg_cycle != nullptr && (E.dbg_cycle_contacts_only ? !vcs.empty() : true);
  std::vector<std::vector<f32>> ring; int cyc_at = velIters, cyc_p = 0;
  auto env_snap = [&]() { std::vector<f32> s; for (int c = 0; c < N; ++c) { const Snap q = snap_of(E.cars[c]); s.insert(s.end(), q.v, q.v + 15); s.insert(s.end(), q.imp, q.imp + 16); }
    for (const VC& vc : vcs) for (int j = 0; j < 2; ++j) { s.push_back(vc.p[j].nImp); s.push_back(vc.p[j].tImp); } return s; };
  if (track_cyc) ring.push_back(env_snap());
  for (int it = 0; it < velIters; ++it) {
    for (int c = 0; c < N; ++c) {
      Snap before; if (track_fix && fix_at[c] == velIters) before = snap_of(E.cars[c]);
      for (int q = 0; q < 4; ++q) joint_solve_velocity(E.cars[c], jord[c][q], h, E.dyn_last(c));
      if (track_fix && fix_at[c] == velIters) { const Snap after = snap_of(E.cars[c]); if (memcmp(&before, &after, sizeof(Snap)) == 0) fix_at[c] = it; }
    }
    for (int oi : cord) contact_solve_velocity(vcs[oi], E.cov);
    if (track_cyc && cyc_at == velIters) {
      const std::vector<f32> cur = env_snap();
      for (int pp = 1; pp <= 8 && pp <= (int)ring.size(); ++pp) {
        const std::vector<f32>& old = ring[ring.size() - pp];
        if (memcmp(old.data(), cur.data(), cur.size() * sizeof(f32)) == 0) { cyc_at = it; cyc_p = pp; break; }
      }
      ring.push_back(cur); if (ring.size() > 8) ring.erase(ring.begin());
    }
  }
  if (track_cyc) E.dbg_cycle[cyc_at * 9 + cyc_p] += 1;
  if (track_fix) for (int c = 0; c < N; ++c) E.dbg_fixed_point[fix_at[c]] += 1;
  for (size_t i = 0; i < S.cur.size(); ++i) for (int j = 0; j < vcs[i].n; ++j) { S.cur[i].m.p[j].nImp = vcs[i].p[j].nImp; S.cur[i].m.p[j].tImp = vcs[i].p[j].tImp; }
  // integrate positions
  for (int c = 0; c < N; ++c) for (int k = 0; k < 5; ++k) {
    Body& b = E.cars[c].b[k];
    V2 tr = h * b.v;
    if (dot(tr, tr) > b2_maxTranslationSquared) { f32 ratio = b2_maxTranslation / length(tr); b.v = ratio * b.v; E.cov[COV_TRANSLATION_CLAMP] += 1; E.dyn_last(c)[DY_TRANSLATION_CLAMP] += 1; }
    f32 rot = h * b.w;
    if (rot * rot > b2_maxRotationSquared) { f32 ratio = b2_maxRotation / fabsf(rot); b.w *= ratio; E.cov[COV_ROTATION_CLAMP] += 1; E.dyn_last(c)[DY_ROTATION_CLAMP] += 1; }
    b.c = b.c + h * b.v; b.a += h * b.w;
  }
  // position iterations + sleep, per island
  for (int root = 0; root < N; ++root) {
    if (isl[root] != root) continue;
    bool positionSolved = false; int sweeps = 0; bool has_contact = false;
    for (const CarContact& C : S.cur) has_contact = has_contact || isl[C.carA] == root;
    for (int it = 0; it < posIters; ++it) {
      sweeps = it + 1;
      f32 before[8][15];                                       // orc_dynamics_coverage: did a failing sweep move the car at all?
      auto poses_of = [](const Car& car, f32* o) { for (int k = 0; k < 5; ++k) { o[3 * k] = car.b[k].c.x; o[3 * k + 1] = car.b[k].c.y; o[3 * k + 2] = car.b[k].a; } };
      for (int c = 0; c < N; ++c) if (isl[c] == root) poses_of(E.cars[c], before[c]);
      E.dbg_pos_iters = std::max(E.dbg_pos_iters, it + 1);
      f32 minSep = 0.0f;
      for (int oi : cord) { const CarContact& C = S.cur[oi]; if (isl[C.carA] != root) continue;
        minSep = std::min(minSep, contact_solve_position(C, E.cars[C.carA].b[fixture_body(C.fixA)], E.cars[C.carB].b[fixture_body(C.fixB)])); }
      bool contactsOkay = minSep >= -3.0f * b2_linearSlop;
      bool jointsOkay = true;
      for (int c = 0; c < N; ++c) if (isl[c] == root)
        for (int q = 0; q < 4; ++q) { bool ok = joint_solve_position(E.cars[c], jord[c][q]); jointsOkay = jointsOkay && ok; }
      if (contactsOkay && jointsOkay) { positionSolved = true; break; }
      for (int c = 0; c < N; ++c) if (isl[c] == root && E.dyn_last(c)[DY_FIXED_AT] == 0) {
        f32 after[15]; poses_of(E.cars[c], after);
        if (memcmp(before[c], after, sizeof(after)) == 0) E.dyn_last(c)[DY_FIXED_AT] = it + 1;
      }
    }
    for (int c = 0; c < N; ++c) if (isl[c] == root) { E.dyn_last(c)[DY_SWEEPS] = sweeps; E.dyn_last(c)[DY_SOLVED] = positionSolved ? 1 : 0; }
    if (has_contact && sweeps == posIters) E.cov[COV_POS_SWEEPS_ALL] += 1;
    f32 minSleepTime = 3.402823466e+38f;
    const f32 linTolSqr = b2_linearSleepTolerance * b2_linearSleepTolerance;
    const f32 angTolSqr = b2_angularSleepTolerance * b2_angularSleepTolerance;
    for (int c = 0; c < N; ++c) if (isl[c] == root) for (int k = 0; k < 5; ++k) {
      Body& b = E.cars[c].b[k];
      b.sync();
      if (b.w * b.w > angTolSqr || dot(b.v, b.v) > linTolSqr) { b.sleepTime = 0.0f; minSleepTime = 0.0f; }
      else { b.sleepTime += h; minSleepTime = std::min(minSleepTime, b.sleepTime); }
    }
    if (minSleepTime >= b2_timeToSleep && positionSolved)
      for (int c = 0; c < N; ++c) if (isl[c] == root) E.dyn_last(c)[DY_SLEPT] = 1;
    if (minSleepTime >= b2_timeToSleep && positionSolved)
      for (int c = 0; c < N; ++c) if (isl[c] == root) for (int k = 0; k < 5; ++k) {
        Body& b = E.cars[c].b[k]; b.awake = false; b.sleepTime = 0.0f; b.v = v2(0, 0); b.w = 0.0f;
      }
  }
  for (int c = 0; c < N; ++c) for (int k = 0; k < 5; ++k) E.cars[c].b[k].force = v2(0, 0);   // ClearForces
}

}  // namespace

extern "C" int orc_debug_pos_iters(void* h) { return ((Env*)h)->dbg_pos_iters; }
// histogram [181] of "first velocity sweep that changed nothing" per (car, step) of this env (180: none); hist == NULL stops the tracking
extern "C" void orc_debug_fixed_point(void* h, long long* hist) { ((Env*)h)->dbg_fixed_point = hist; }
// histogram [181][9] of (first sweep whose end state repeats the state p sweeps earlier, p) per step of this env ((180, 0): none); contacts_only:
// count only the steps with touching car<->car contacts
extern "C" void orc_debug_cycle(void* h, long long* hist, int contacts_only) { ((Env*)h)->dbg_cycle = hist; ((Env*)h)->dbg_cycle_contacts_only = contacts_only; }
extern "C" int orc_num_car_contacts(void* h) { return (int)store_of(*(Env*)h).cur.size(); }
// The env's touching contacts after the last step, in the order they were solved, as the product's manifold store holds them
// (multi_car_racing_amd/csrc/k_carcontacts.h: the record layout): out[0] = count, out[1] = 1 if the cap dropped pairs in that step,
// out[2..3] = each car's joint order (2 bits per position, 8 bits per car), then 16 words per contact: key = carA | fixA << 4 | carB << 8 |
// fixB << 12, type | n << 8, localNormal, localPoint, two points of (local x, local y, nImp, tImp, id); the words of a point the manifold
// does not have are 0.  Writes at most `cap` words; returns the count.
extern "C" int orc_get_car_contacts(void* h, uint32_t* out, int cap) {
  Env& E = *(Env*)h; const ContactStore& S = store_of(E);
  const int n = (int)S.cur.size();
  std::vector<uint32_t> w(4 + (size_t)n * 16, 0u);
  auto bits = [](f32 v) { uint32_t u; memcpy(&u, &v, 4); return u; };
  w[0] = (uint32_t)n; w[1] = (E.contact_cap > 0 && S.candidates > E.contact_cap) ? 1u : 0u;
  if ((int)S.cord.size() == n) {
    unsigned long long jo = 0ull;
    for (int c = 0; c < E.N; ++c) for (int q = 0; q < 4; ++q) jo |= (unsigned long long)(S.jord[c][q] & 3) << (c * 8 + 2 * q);
    w[2] = (uint32_t)jo; w[3] = (uint32_t)(jo >> 32);
    for (int i = 0; i < n; ++i) {
      const CarContact& C = S.cur[S.cord[i]]; uint32_t* d = &w[4 + (size_t)i * 16];
      d[0] = (uint32_t)C.carA | ((uint32_t)C.fixA << 4) | ((uint32_t)C.carB << 8) | ((uint32_t)C.fixB << 12);
      d[1] = (uint32_t)C.m.type | ((uint32_t)C.m.n << 8);
      d[2] = bits(C.m.localNormal.x); d[3] = bits(C.m.localNormal.y); d[4] = bits(C.m.localPoint.x); d[5] = bits(C.m.localPoint.y);
      for (int j = 0; j < C.m.n; ++j) { uint32_t* q = d + 6 + j * 5; q[0] = bits(C.m.p[j].local.x); q[1] = bits(C.m.p[j].local.y); q[2] = bits(C.m.p[j].nImp); q[3] = bits(C.m.p[j].tImp); q[4] = C.m.p[j].id; }
    }
  }
  for (size_t i = 0; i < w.size() && (int)i < cap; ++i) out[i] = w[i];
  return n;
}
// Coverage of the contact code by this env since the last reset of the counters: out[ORC_COV_ROWS] (oracle.py: COVERAGE_ROWS names them)
extern "C" int orc_contact_coverage(void* h, long long* out, int reset) {
  Env& E = *(Env*)h;
  for (int i = 0; i < ORC_COV_ROWS; ++i) { out[i] = E.cov[i]; if (reset) E.cov[i] = 0; }
  return COV_ROWS;
}
// What the per-car dynamics reached (mcr_oracle.cpp: DY_*): out[N][2][DY_ROWS] — each car's rows of the last step, then their totals since the
// counters were last reset (reset != 0 clears the totals after the read).  Returns DY_ROWS.
extern "C" int orc_dynamics_coverage(void* h, long long* out, int reset) {
  Env& E = *(Env*)h;
  for (size_t i = 0; i < E.dyn.size(); ++i) out[i] = E.dyn[i];
  if (reset) for (int c = 0; c < E.N; ++c) std::fill(E.dyn_last(c) + DY_ROWS, E.dyn_last(c) + 2 * DY_ROWS, 0LL);
  return DY_ROWS;
}
// 0 (default): no cap.  cap > 0: THE DROP RULE of the header, the product's MCR_CC_MAX
extern "C" void orc_set_contact_cap(void* h, int cap) { ((Env*)h)->contact_cap = cap < 0 ? 0 : cap; }
