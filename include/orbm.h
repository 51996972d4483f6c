/* orbm.h -- C ABI of the MI355X-native ORB matcher primitives (drop-in path for ORB_SLAM3::ORBmatcher
 * and the Hamming association loops of Frame).
 *
 * The reference has no FFI layer; its boundary is the C++ class ORBmatcher (include/ORBmatcher.h:35-111)
 * whose search methods walk Frame / KeyFrame / MapPoint object graphs.  The C++ facade
 * (orb-slam3_amd/facade/ORBmatcher.h) flattens those objects into the plain arrays below, runs the
 * data-parallel distance phase on the GPU and replays the order-dependent "claim" bookkeeping on the host
 * (SURVEY 8(a) M-rows, 8(b)).
 *
 * Conventions as in orbx.h: negative return = ORBM_E_*, caller-owned buffers, no CPU fallback.
 * Descriptors are rows of 32 bytes (256 bit), exactly cv::Mat(n,32,CV_8U) rows.
 */
#ifndef ORBM_H_
#define ORBM_H_
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

enum { ORBM_OK = 0, ORBM_E_INVALID = -2, ORBM_E_CAPACITY = -3, ORBM_E_HIP = -5 };
enum { ORBM_HOST = 0, ORBM_DEVICE = 1 };
enum { ORBM_TH_HIGH = 100, ORBM_TH_LOW = 50, ORBM_HISTO_LENGTH = 30 };   /* ORBmatcher.cc:36-38 */
/* match[] values of the searches that write into an EXISTING Frame::mvpMapPoints (M4, M5 and the fisheye twin of M4):
 * >= 0 the query matched here; ORBM_NO_MATCH the slot was not touched; ORBM_MATCH_PRUNED the slot was assigned and then culled
 * by the rotation-consistency check -- the reference leaves NULL there (ORBmatcher.cc:2700-2708, 2843-2847), whatever the slot
 * held before, so a wrapper must clear it. */
enum { ORBM_NO_MATCH = -1, ORBM_MATCH_PRUNED = -2 };

typedef struct orbm orbm_t;       /* owns a stream + scratch on one device */
int orbm_create(orbm_t** out, int device_id);
void orbm_destroy(orbm_t*);
const char* orbm_last_error(void);
int orbm_sync(orbm_t*);
void* orbm_stream(const orbm_t*);
/* run the matcher's kernels on the caller's hipStream_t (e.g. orbx_stream() of the extractor whose results they read: one
 * stream, no cross-stream event waits); NULL returns to the handle's own stream */
int orbm_set_stream(orbm_t*, void* stream);

/* M0  ORBmatcher::DescriptorDistance (ORBmatcher.cc:2911-2931): host-side scalar, 4 x popcount64 */
int orbm_hamming(const uint8_t* a, const uint8_t* b);

/* M1  ORBmatcher::ComputeThreeMaxima on bin sizes (ORBmatcher.cc:2863-2905) */
void orbm_three_maxima(const int* bin_sizes, int L, int* ind3);

/* M16 dense brute-force 2-NN (cv::BFMatcher(NORM_HAMMING).knnMatch k=2 in Frame::ComputeStereoFishEyeMatches,
 * Frame.cc:1440-1480).  Batched over `npairs` independent (query set, train set) pairs.
 *   q, t     : [npairs][q_stride rows][32] / [npairs][t_stride rows][32] descriptors (host or device: `space`)
 *   nq, nt   : per-pair row counts, int32[npairs] in the same space
 *   idx2/dist2 : [npairs][q_stride][2] int32, same space; idx -1 / dist -1 when fewer than k train rows.
 * Ties: lower train index first (the oracle's normative order). */
int orbm_knn2_batch(orbm_t*, int space, const uint8_t* q, int q_stride, const int32_t* nq,
                    const uint8_t* t, int t_stride, const int32_t* nt, int npairs,
                    int32_t* idx2, int32_t* dist2);
/* M16 with the reference's acceptance test in the kernel's epilogue: good[npairs][q_stride] (device) = 1 where the query has two
 * neighbours and `(*it)[0].distance < (*it)[1].distance * ratio` holds as Frame.cc:1465 evaluates it (float distances, double
 * product; the reference's ratio is 0.7), else 0.  idx2 / dist2 as orbm_knn2_batch_async.  Device pointers, enqueue only. */
int orbm_knn2_ratio_batch_async(orbm_t*, const uint8_t* q, int q_stride, const int32_t* nq,
                                const uint8_t* t, int t_stride, const int32_t* nt, int npairs, double ratio,
                                int32_t* idx2, int32_t* dist2, uint8_t* good);
/* async form (device pointers only, no sync) -- the timed body of bench.py */
int orbm_knn2_batch_async(orbm_t*, const uint8_t* q, int q_stride, const int32_t* nq,
                          const uint8_t* t, int t_stride, const int32_t* nt, int npairs, int max_nt,
                          int32_t* idx2, int32_t* dist2);
int orbm_last_timing(orbm_t*, float* ms);

/* ------------------------------------------------------------------------------------------------------------
 * Flattened Frame / KeyFrame views.  The reference's searches walk Frame/KeyFrame/MapPoint object graphs; the C++
 * facade copies the few fields each search reads into these plain arrays.  All pointers below are
 * HOST pointers; every search uploads them, runs the data-parallel phase (grid gather + 256-bit Hamming) on the
 * GPU and replays the reference's order-dependent bookkeeping on the host with the device-computed distances.
 * ------------------------------------------------------------------------------------------------------------ */
#define ORBM_GRID_COLS 64     /* Frame.h:37 */
#define ORBM_GRID_ROWS 48     /* Frame.h:38 */

typedef struct { float x, y, size, angle, response; int32_t octave, class_id; } orbm_kp_t;   /* == cv::KeyPoint */

typedef struct {
    int32_t n;                 /* N keypoints */
    const orbm_kp_t* kps;      /* mvKeysUn (Frame.h) */
    const uint8_t* desc;       /* mDescriptors rows */
    const float* uright;       /* mvuRight or NULL */
    float min_x, min_y, inv_w, inv_h;   /* mnMinX, mnMinY, mfGridElementWidthInv, mfGridElementHeightInv */
    const int32_t* grid_start; /* [64*48+1] CSR, cell = ix*48+iy == mGrid[ix][iy] */
    const int32_t* grid_idx;   /* keypoint indices in insertion order */
} orbm_frame_t;

/* M14  Frame::AssignFeaturesToGrid + PosInGrid (Frame.cc:446-480, 883-899) on the GPU.
 * grid_start[3073], grid_idx[n] are host outputs; returns the number of keypoints placed.
 * The limit of the three grid builders (this call, orbm_frame_create, orbm_grid_build_batch_async): n, or cap, <= 65535 keypoints per
 * frame -- the batched searches' own limit, so every pool row they accept has a grid from here.  Above it this call and
 * orbm_frame_create return ORBM_E_CAPACITY, orbm_grid_build_batch_async ORBM_E_INVALID.  Up to 8192 keypoints a counting sort over the
 * 3072 cells, up to 32768 a bitonic sort of cell << 16 | index keys in LDS, above that the counting sort again with every cell list of
 * more than 64 entries put in order by the whole workgroup (155 666 B of LDS at 65535); the result is the same CSR in each. */
int orbm_grid_build(orbm_t*, const orbm_kp_t* kps, int n, float min_x, float min_y, float inv_w, float inv_h,
                    int32_t* grid_start, int32_t* grid_idx);

/* M14  Frame::GetFeaturesInArea (Frame.cc:784-871) for a batch of windows, with the Hamming distance of every
 * returned keypoint to the window's query descriptor.  Candidates come out in the reference's order
 * (ix, iy, insertion).  q_* arrays have nq entries; er_max < 0 disables the stereo gate
 * (`uright[i] > 0 && fabs(ur - uright[i]) > er_max` -> skipped, ORBmatcher.cc:107-117, 2569-2576).
 * out_idx/out_dist: [nq][cap]; out_cnt[nq].  Returns 0, or ORBM_E_CAPACITY if any window overflowed `cap`. */
int orbm_window_candidates(orbm_t*, const orbm_frame_t* f, int nq, const float* qx, const float* qy, const float* qr,
                           const int32_t* min_level, const int32_t* max_level, const float* q_ur, const float* q_er_max,
                           const uint8_t* qdesc, int cap, int32_t* out_cnt, int32_t* out_idx, int32_t* out_dist);

/* M4  ORBmatcher::SearchByProjection(Frame& Cur, const Frame& Last, th, bMono) (ORBmatcher.cc:2469-2711),
 * mono / rectified-stereo path.  Per last-frame feature i: valid[i] (MapPoint present, not an outlier, invzc >= 0,
 * projection inside the image: decided by the caller's camera model), projection (u,v), invzc, octave, angle,
 * MapPoint descriptor, mp_obs[i] = pMP->Observations() > 0.  cur_blocked[i2] = Cur.mvpMapPoints[i2] already holds a
 * MapPoint with observations.  match[i2] = index of the last-frame feature whose MapPoint lands on i2, or -1. */
int orbm_search_by_projection_frame(orbm_t*, const orbm_frame_t* cur, const uint8_t* cur_blocked, const float* scale_factors,
                                    int nq, const uint8_t* valid, const float* u, const float* v, const float* invzc,
                                    const int32_t* octave, const float* angle, const uint8_t* qdesc, const uint8_t* mp_obs,
                                    float th, int forward, int backward, float mbf, int check_ori, int32_t* match);

/* M3  ORBmatcher::SearchByProjection(Frame&, const vector<MapPoint*>&, th, ...) (ORBmatcher.cc:45-239), left camera */
int orbm_search_by_projection_points(orbm_t*, const orbm_frame_t* f, const uint8_t* blocked, const float* scale_factors,
                                     int nq, const uint8_t* in_view, const float* px, const float* py, const float* pxr,
                                     const float* view_cos, const int32_t* level, const uint8_t* qdesc, const uint8_t* mp_obs,
                                     float th, float nnratio, int32_t* match);

/* ---- frames resident in HBM.  Tracking runs 2-4 searches on the same Frame (TrackWithMotionModel / TrackReferenceKeyFrame,
 * then SearchLocalPoints; Tracking.cc:3002-3211, 3867-3891): orbm_frame_create uploads keypoints, descriptors and mvuRight
 * ONCE (space = ORBM_HOST), or adopts device arrays without copying them (space = ORBM_DEVICE: an extractor's result block,
 * orbx_result_device -- they must stay valid while the frame lives), and builds the 64 x 48 grid (M14) on the device (n <= 65535,
 * the builders' limit at orbm_grid_build).  The
 * *_resident searches then send only their queries and get back, per query, the candidate count and the 8 best (distance,
 * visiting-order) candidates -- all the claim replay can look at unless every one of them is blocked, in which case the call
 * falls back to the full candidate lists by itself.  Same arguments and results as M4 / M3 above. */
typedef struct orbm_dframe orbm_dframe_t;
int orbm_frame_create(orbm_t*, int space, int n, const orbm_kp_t* kps, const uint8_t* desc, const float* uright,
                      float min_x, float min_y, float inv_w, float inv_h, orbm_dframe_t** out);
void orbm_frame_destroy(orbm_dframe_t*);
int orbm_frame_size(const orbm_dframe_t*);
int orbm_search_by_projection_frame_resident(orbm_t*, const orbm_dframe_t* cur, const uint8_t* cur_blocked, const float* scale_factors,
                                             int nq, const uint8_t* valid, const float* u, const float* v, const float* invzc,
                                             const int32_t* octave, const float* angle, const uint8_t* qdesc, const uint8_t* mp_obs,
                                             float th, int forward, int backward, float mbf, int check_ori, int32_t* match);
int orbm_search_by_projection_points_resident(orbm_t*, const orbm_dframe_t* f, const uint8_t* blocked, const float* scale_factors,
                                              int nq, const uint8_t* in_view, const float* px, const float* py, const float* pxr,
                                              const float* view_cos, const int32_t* level, const uint8_t* qdesc, const uint8_t* mp_obs,
                                              float th, float nnratio, int32_t* match);

/* M5  ORBmatcher::SearchByProjection(Frame&, KeyFrame*, sAlreadyFound, th, ORBdist) (ORBmatcher.cc:2723-2852), relocalisation.
 * valid[i] folds the caller-side gates (MapPoint present / not bad / not already found / projection in bounds /
 * distance invariance); level[i] = PredictScale; blocked[i2] = CurrentFrame.mvpMapPoints[i2] != NULL. */
int orbm_search_by_projection_kf(orbm_t*, const orbm_frame_t* cur, const uint8_t* blocked, const float* scale_factors,
                                 int nq, const uint8_t* valid, const float* u, const float* v, const int32_t* level,
                                 const float* angle, const uint8_t* qdesc, float th, int orb_dist, int check_ori, int32_t* match);

/* M6  ORBmatcher::SearchByProjection(KeyFrame*, Scw, vpPoints, vpMatched, th, ratioHamming) (ORBmatcher.cc:549-679; the
 * +vpPointsKFs overload :681-797 matches identically).  valid[i] folds the caller-side Sim3 projection gates;
 * matched_in[idx] = vpMatched[idx] != NULL; match[idx] = iMP or -1.  `kf` is the KeyFrame's view (KeyFrame.h:243-250,319). */
int orbm_search_by_projection_sim3(orbm_t*, const orbm_frame_t* kf, const uint8_t* matched_in, const float* scale_factors,
                                   int nq, const uint8_t* valid, const float* u, const float* v, const int32_t* level,
                                   const uint8_t* qdesc, int th, float ratio_hamming, int32_t* match);

/* M13 search core of ORBmatcher::Fuse (ORBmatcher.cc:1823-2049: chi2_gate = 1; Sim3 variant :2051-2199: chi2_gate = 0).
 * best_idx[i] = KeyFrame feature MapPoint i fuses into, or -1; AddObservation / Replace stay with the caller. */
int orbm_fuse(orbm_t*, const orbm_frame_t* kf, const float* scale_factors, const float* inv_sigma2,
              int nq, const uint8_t* valid, const float* u, const float* v, const float* ur, const int32_t* level,
              const uint8_t* qdesc, float th, int chi2_gate, int32_t* best_idx);

/* M13 ORBmatcher::SearchBySim3 (ORBmatcher.cc:2201-2467): two independent guided searches (KeyFrame 1's MapPoints in
 * KeyFrame 2 and vice versa; projections + gates done by the caller) and the mutual-consistency check.
 * matches12[i1] = idx2 or -1; returns nFound. */
int orbm_search_by_sim3(orbm_t*, const orbm_frame_t* kf1, const orbm_frame_t* kf2, const float* sf1, const float* sf2,
                        const uint8_t* valid1, const float* u1, const float* v1, const int32_t* level1, const uint8_t* qdesc1,
                        const uint8_t* valid2, const float* u2, const float* v2, const int32_t* level2, const uint8_t* qdesc2,
                        float th, int32_t* matches12);

/* ---- fisheye stereo (Nleft != -1): left / right keypoints in separate arrays and grids (mvKeys + mGrid, mvKeysRight +
 * mGridRight); MapPoint slots [0,Nleft) and [Nleft, Nleft+Nright) are reported as match_l / match_r ---- */
/* M4 with the right-camera block (ORBmatcher.cc:2615-2680); (ur, vr) = projection into the right camera */
int orbm_search_by_projection_frame_fisheye(orbm_t*, const orbm_frame_t* cur_l, const orbm_frame_t* cur_r,
                                            const uint8_t* blocked_l, const uint8_t* blocked_r, const float* scale_factors,
                                            int nq, const uint8_t* valid, const float* u, const float* v, const float* ur, const float* vr,
                                            const int32_t* octave, const float* angle, const uint8_t* qdesc, const uint8_t* mp_obs,
                                            float th, int forward, int backward, int check_ori, int32_t* match_l, int32_t* match_r);
/* M3 with the right-camera block (ORBmatcher.cc:170-236) and the mvLeftToRightMatch / mvRightToLeftMatch cross
 * assignments (:152-157, :222-226); l2r[nL], r2l[nR] hold -1 or the partner index */
int orbm_search_by_projection_points_fisheye(orbm_t*, const orbm_frame_t* f_l, const orbm_frame_t* f_r,
                                             const uint8_t* blocked_l, const uint8_t* blocked_r,
                                             const int32_t* l2r, const int32_t* r2l, const float* scale_factors,
                                             int nq, const uint8_t* in_view, const float* px, const float* py, const float* view_cos, const int32_t* level,
                                             const uint8_t* in_view_r, const float* pxr, const float* pyr, const float* view_cos_r, const int32_t* level_r,
                                             const uint8_t* qdesc, const uint8_t* mp_obs, float th, float nnratio, int32_t* match_l, int32_t* match_r);
/* M7 with F.Nleft != -1 (ORBmatcher.cc:405-426, 471-500): frame features [0,nleft) are left, the rest right */
int orbm_search_by_bow_fisheye(orbm_t*, int nkf, const orbm_kp_t* kps_kf, const uint8_t* desc_kf, const uint8_t* kf_good,
                               int nnk, const int32_t* nodes_k, const int32_t* start_k, const int32_t* idx_k,
                               int nf, int nleft, const orbm_kp_t* kps_f, const uint8_t* desc_f,
                               int nnf, const int32_t* nodes_f, const int32_t* start_f, const int32_t* idx_f,
                               float nnratio, int check_ori, int32_t* f_match);

/* M9  ORBmatcher::SearchForInitialization (ORBmatcher.cc:799-943); prev_matched_xy is updated in place */
int orbm_search_for_initialization(orbm_t*, const orbm_frame_t* f1, const orbm_frame_t* f2, float* prev_matched_xy,
                                   int window, float nnratio, int check_ori, int32_t* matches12);

/* M10 ORBmatcher::SearchForTriangulation_ (ORBmatcher.cc:1388-1629), pinhole cameras.  FeatureVectors are CSR:
 * `nodes` ascending, start[nn+1], idx[].  F12: row-major 3x3 (what Pinhole::epipolarConstrain_ builds,
 * Pinhole.cpp:273-280); (epx,epy) the epipole in image 2 (ORBmatcher.cc:1399-1400). */
int orbm_search_for_triangulation(orbm_t*, int n1, const orbm_kp_t* kps1, const uint8_t* desc1, const uint8_t* has_mp1, const float* uright1,
                                  int nn1, const int32_t* nodes1, const int32_t* start1, const int32_t* idx1,
                                  int n2, const orbm_kp_t* kps2, const uint8_t* desc2, const uint8_t* has_mp2, const float* uright2,
                                  int nn2, const int32_t* nodes2, const int32_t* start2, const int32_t* idx2,
                                  const float* F12, float epx, float epy, const float* scale_factors2, const float* level_sigma2_2,
                                  int only_stereo, int coarse, int check_ori, int32_t* matches12);

/* M7  ORBmatcher::SearchByBoW(KeyFrame*, Frame&, ...) (ORBmatcher.cc:314-547), Nleft == -1.  f_match[iF] = KF index or -1 */
int orbm_search_by_bow(orbm_t*, int nkf, const orbm_kp_t* kps_kf, const uint8_t* desc_kf, const uint8_t* kf_good,
                       int nnk, const int32_t* nodes_k, const int32_t* start_k, const int32_t* idx_k,
                       int nf, const orbm_kp_t* kps_f, const uint8_t* desc_f,
                       int nnf, const int32_t* nodes_f, const int32_t* start_f, const int32_t* idx_f,
                       float nnratio, int check_ori, int32_t* f_match);

/* M8  ORBmatcher::SearchByBoW(KeyFrame*, KeyFrame*, vpMatches12) (ORBmatcher.cc:955-1105); matches12[idx1] = idx2 or -1 */
int orbm_search_by_bow_kf(orbm_t*, int n1, const orbm_kp_t* kps1, const uint8_t* desc1, const uint8_t* good1,
                          int nn1, const int32_t* nodes1, const int32_t* start1, const int32_t* idx1,
                          int n2, const orbm_kp_t* kps2, const uint8_t* desc2, const uint8_t* good2,
                          int nn2, const int32_t* nodes2, const int32_t* start2, const int32_t* idx2,
                          float nnratio, int check_ori, int32_t* matches12);

/* M11 ORBmatcher::SearchForTriangulation, cv::Mat F12 overload (ORBmatcher.cc:1107-1386): as M10 but vbMatched2 is kept
 * (set :1319, cleared by the orientation cull :1366) and the histogram factor is 30/360 (:1166). */
int orbm_search_for_triangulation_legacy(orbm_t*, int n1, const orbm_kp_t* kps1, const uint8_t* desc1, const uint8_t* has_mp1, const float* uright1,
                                  int nn1, const int32_t* nodes1, const int32_t* start1, const int32_t* idx1,
                                  int n2, const orbm_kp_t* kps2, const uint8_t* desc2, const uint8_t* has_mp2, const float* uright2,
                                  int nn2, const int32_t* nodes2, const int32_t* start2, const int32_t* idx2,
                                  const float* F12, float epx, float epy, const float* scale_factors2, const float* level_sigma2_2,
                                  int only_stereo, int coarse, int check_ori, int32_t* matches12);

/* M10 with a second camera (pKF1->mpCamera2, ORBmatcher.cc:1413-1426, 1526-1557) and M12
 * (ORBmatcher::SearchForTriangulation(+vMatchedPoints), ORBmatcher.cc:1632-1821).  Both are the M10 bucket search with the
 * geometric gate supplied by the camera model (GeometricCamera::epipolarConstrain_ :1552, ::matchAndtriangulate :1729 —
 * KannalaBrandt8 unprojects, triangulates with cv::SVD and tests the reprojection, KannalaBrandt8.cpp:356-361, 363-472,
 * 559-700; Pinhole::matchAndtriangulate is `return false`, Pinhole.h:88-91), no epipole
 * gate (:1517 needs !mpCamera2; M12 has none) and no stereo flags (bStereo is false with mpCamera2, :1462; M12 ignores
 * bOnlyStereo).  The gate stays with the caller: `gate(user, idx1, idx2)` is called exactly where the reference calls the
 * camera model — after the MapPoint and `dist <= TH_LOW && dist <= bestDist` tests, in bucket order — and a nonzero
 * return accepts the pair, so a callback that records its last accepted x3D per idx1 reproduces M12's vMatchedPoints.
 * kps1/kps2 are the N-long keypoint arrays the reference indexes (mvKeysUn, or mvKeys followed by mvKeysRight when
 * NLeft != -1, :1467-1469); histogram factor 1/30 (:1441, :1672).  Descriptor distances are computed on the GPU. */
typedef int (*orbm_pair_gate_fn)(void* user, int idx1, int idx2);
int orbm_search_for_triangulation_gated(orbm_t*, int n1, const orbm_kp_t* kps1, const uint8_t* desc1, const uint8_t* has_mp1,
                                        int nn1, const int32_t* nodes1, const int32_t* start1, const int32_t* idx1,
                                        int n2, const orbm_kp_t* kps2, const uint8_t* desc2, const uint8_t* has_mp2,
                                        int nn2, const int32_t* nodes2, const int32_t* start2, const int32_t* idx2,
                                        orbm_pair_gate_fn gate, void* user, int check_ori, int32_t* matches12);

/* ---- batched, DEVICE-resident forms: frame-to-frame tracking chained behind orbx_extract_batch_async with no host round
 * trip (kps/desc/counts are the extractor's result block, orbx_result_device; all pointers are device pointers).
 * orbm_grid_build_batch_async: M14 for every frame of the block; grid_start [nframes][3073], grid_idx [nframes][cap]; cap <= 65535
 * (the builders' limit, at orbm_grid_build); frame f holds min(counts[f], cap) keypoints.
 * orbm_track_window_batch_async: for pair p the keypoints of frame q_first+p search frame t_first+p inside the mono
 * SearchByProjection window (centre (x+dx, y+dy), radius th*scale[octave], levels octave-1..octave+1,
 * ORBmatcher.cc:2543-2549): first-minimum best index/distance and runner-up distance per keypoint, [npairs][cap].
 * This is the claim-free, data-parallel part; the final matches of the batch: orbm_search_by_projection_batch_async. */
/* orbm_search_by_projection_batch_async: M4 SearchByProjection(CurrentFrame, LastFrame, th, bMono = true) END TO END on the device
 * for `npairs` frame pairs of one result block (ORBmatcher.cc:2469-2711, the monocular branch: no mvuRight gate, window levels
 * octave-1..octave+1).  Pair p: the keypoints of frame q_first+p play LastFrame's MapPoints in index order -- every one valid,
 * projected to (x+dx, y+dy), carrying its own descriptor, octave and angle -- and search frame t_first+p through its grid.
 * t_blocked [frames][cap] (device, indexed by FRAME id; NULL = none): slots of the searched frame that already hold a MapPoint
 * with observations (:2565-2567).  q_obs [frames][cap] (NULL = all 1): pMP->Observations() > 0 of the query's MapPoint, i.e.
 * whether its assignment blocks later queries.  The claim sequence, `bestDist <= TH_HIGH`, the rotation histogram and the
 * ComputeThreeMaxima cull (:2595-2605, 2690-2708) run in query order on the device.  Outputs (device): match [npairs][cap] =
 * query index assigned to that slot of the searched frame, ORBM_NO_MATCH or ORBM_MATCH_PRUNED -- the same row
 * orbm_search_by_projection_frame returns for the pair --, nmatches [npairs] = its return value.  Enqueue-only (capturable;
 * the first call with a larger batch grows the handle's scratch and must run outside a capture).  cap <= ~16 000 keypoint slots per
 * frame (the claim replay keeps 4 B per slot in 64 KB of LDS); ORBM_E_INVALID above. */
int orbm_search_by_projection_batch_async(orbm_t*, const orbm_kp_t* kps, const uint8_t* desc, const int32_t* counts, int cap,
                                          const int32_t* grid_start, const int32_t* grid_idx,
                                          float min_x, float min_y, float inv_w, float inv_h,
                                          int q_first, int t_first, int npairs, float th, const float* scale_factors_host, int nlevels,
                                          float dx, float dy, const uint8_t* t_blocked, const uint8_t* q_obs, int check_orientation,
                                          int32_t* match, int32_t* nmatches);
int orbm_grid_build_batch_async(orbm_t*, const orbm_kp_t* kps, const int32_t* counts, int nframes, int cap,
                                float min_x, float min_y, float inv_w, float inv_h, int32_t* grid_start, int32_t* grid_idx);
int orbm_track_window_batch_async(orbm_t*, const orbm_kp_t* kps, const uint8_t* desc, const int32_t* counts, int cap,
                                  const int32_t* grid_start, const int32_t* grid_idx,
                                  float min_x, float min_y, float inv_w, float inv_h,
                                  int q_first, int t_first, int npairs, float th, const float* scale_factors_host, int nlevels,
                                  float dx, float dy, int32_t* best_idx, int32_t* best_dist, int32_t* second_dist);
/* orbm_search_by_projection_points_batch_async: M3 SearchByProjection(Frame, vector<MapPoint*>, th, bFarPoints, thFarPoints) --
 * Tracking::SearchLocalPoints -- END TO END on the device for `nframes` frames of one result block (ORBmatcher.cc:45-166, the
 * left-camera part; the Nleft != -1 block :170-236 is orbm_search_by_projection_points_fisheye_batch_async below).  Frame f of the call is
 * block frame t_first+f; it is searched through its grid (orbm_grid_build_batch_async over the block, indexed by block frame id).
 * Every other per-frame array has one row per frame of the call: uright [nframes][cap] (mvuRight, e.g. orbm_stereo_batch_async with
 * first_l == t_first; NULL = no stereo gate), t_blocked [nframes][cap] (mvpMapPoints[i] && Observations() > 0; NULL = none).
 * The queries are the local map points: nq [nframes] of them per frame, rows of q_stride entries -- in_view, proj_x, proj_y,
 * proj_xr (read only with uright), view_cos, level exactly as orbm_is_in_frustum(ORBM_DEVICE) writes them into row f; depth (NULL
 * = bFarPoints off) skips a point with depth > th_far.  qdesc [..][32] and mp_obs [..] (Observations() > 0) are per frame rows
 * too, or ONE row shared by every frame when q_shared != 0.  A point that is not in view, beyond th_far or whose level is outside
 * [0, nlevels) reads nothing else of its row.  Window, stereo gate, best / second, TH_HIGH and the same-level ratio rule are those
 * of orbm_search_by_projection_points; claims run in query order: an assignment may overwrite the slot of a point without
 * observations and counts again, only a point with observations blocks its slot for later ones.  Outputs (device): match
 * [nframes][cap] = query index or ORBM_NO_MATCH (the row orbm_search_by_projection_points returns, padded to cap), nmatches
 * [nframes] = its return value.  All pointers are device pointers except scale_factors_host.  Enqueue-only: after one eager call
 * the same or a smaller shape allocates nothing and can be captured (orbx_capture_begin).  ORBM_E_INVALID: a NULL array, a count
 * < 1; ORBM_E_CAPACITY: cap > 65535, q_stride > ORBM_LP_MAX_QUERIES, nlevels > 12, nframes > 65535.  Nothing is enqueued then. */
enum { ORBM_LP_MAX_QUERIES = 1 << 20 };
int orbm_search_by_projection_points_batch_async(orbm_t*, const orbm_kp_t* kps, const uint8_t* desc, const int32_t* counts, int cap,
                                                 const int32_t* grid_start, const int32_t* grid_idx,
                                                 float min_x, float min_y, float inv_w, float inv_h, int t_first, int nframes,
                                                 const float* uright, const uint8_t* t_blocked, const int32_t* nq, int q_stride,
                                                 const uint8_t* in_view, const float* proj_x, const float* proj_y, const float* proj_xr,
                                                 const float* view_cos, const int32_t* level, const float* depth, float th_far,
                                                 const uint8_t* qdesc, const uint8_t* mp_obs, int q_shared,
                                                 float th, float nnratio, const float* scale_factors_host, int nlevels,
                                                 int32_t* match, int32_t* nmatches);
/* orbm_search_by_projection_frame_batch_async: M4 SearchByProjection(CurrentFrame, LastFrame, th, bMono) -- Tracking::TrackWithMotionModel
 * -- END TO END on the device for `npairs` pairs (ORBmatcher.cc:2469-2612 and the rotation check :2686-2708, the Nleft == -1 part; the
 * fisheye right-camera block is orbm_search_by_projection_frame_fisheye_batch_async).  Pair p searches block frame t_first+p through its grid
 * (orbm_grid_build_batch_async over the block, indexed by block frame id).  Per pair rows: uright [npairs][cap] (mvuRight, e.g.
 * orbm_stereo_batch_async with first_l == t_first; NULL = no stereo gate, invzc is then not read and may be NULL), t_blocked
 * [npairs][cap] (the slot holds a MapPoint with Observations() > 0; NULL = none), dir [npairs] (0 = levels o-1..o+1, 1 = bForward:
 * levels >= o, 2 = bBackward: levels <= o; other values read as 0; NULL = all 0; orbm_project_last_frame_batch_async writes it).
 * The queries are the LastFrame MapPoints: nq [npairs] of them per pair in rows of q_stride entries -- valid, u, v, invzc, octave,
 * angle (the LastFrame keypoint's), qdesc [..][32] (the MapPoint's descriptor) and mp_obs (Observations() > 0).  A query that is not
 * valid, or whose octave lies outside [0, nlevels), reads nothing else of its row.  Semantics per pair are exactly those of
 * orbm_search_by_projection_frame: window th * scale[octave], stereo gate ur = u - mbf * invzc, first candidate of least distance not
 * blocked, bestDist <= TH_HIGH; claims in query order, an assignment may overwrite the slot of a query without observations and counts
 * again, only mp_obs blocks a slot for later queries; check_orientation applies the rotation histogram and its three-maxima cull
 * (culled slots ORBM_MATCH_PRUNED).  retry_below > 0: every pair whose count is below it is searched again at 2 * th from an empty
 * frame (no blocked slots, Tracking.cc:3213-3221), on the device; that row and count replace the first ones and retried[p] = 1
 * (retried [npairs] or NULL; 0 for the other pairs).  Outputs (device): match [npairs][cap] (the row orbm_search_by_projection_frame
 * returns, padded with ORBM_NO_MATCH to cap), nmatches [npairs] (its return value).  All pointers are device pointers except
 * scale_factors_host.  Enqueue-only: after one eager call the same or a smaller shape allocates nothing and can be captured
 * (orbx_capture_begin).  ORBM_E_INVALID: a NULL required array, a count < 1, t_first or retry_below < 0; ORBM_E_CAPACITY: cap >
 * 65535, q_stride > ORBM_LP_MAX_QUERIES, nlevels > 12, npairs > 65535.  Nothing is enqueued then. */
int orbm_search_by_projection_frame_batch_async(orbm_t*, const orbm_kp_t* kps, const uint8_t* desc, const int32_t* counts, int cap,
                                                const int32_t* grid_start, const int32_t* grid_idx,
                                                float min_x, float min_y, float inv_w, float inv_h, int t_first, int npairs,
                                                const float* uright, float mbf, const uint8_t* t_blocked, const uint8_t* dir,
                                                const int32_t* nq, int q_stride, const uint8_t* valid, const float* u, const float* v,
                                                const float* invzc, const int32_t* octave, const float* angle, const uint8_t* qdesc,
                                                const uint8_t* mp_obs, float th, int retry_below, const float* scale_factors_host, int nlevels,
                                                int check_orientation, int32_t* match, int32_t* nmatches, uint8_t* retried);
/* orbm_search_by_projection_frame_fisheye_batch_async: M4 SearchByProjection(CurrentFrame, LastFrame, th, bMono) with CurrentFrame.Nleft
 * != -1 -- Tracking::TrackWithMotionModel on a fisheye stereo rig -- END TO END on the device for `npairs` pairs (ORBmatcher.cc:2469-2711,
 * the right-camera block :2615-2680 included).  One pool of rows of `cap` slots (kps, desc, counts and the grid of
 * orbm_grid_build_batch_async over it: an extractor result block or a caller-gathered array in that layout); pair p searches left row
 * first_l+p (mvKeys, mGrid) and right row first_r+p (mvKeysRight, mGridRight), paired as orbm_stereo_batch_async pairs them; both grids
 * share min_x, min_y, inv_w, inv_h (PosInGrid, Frame.cc:883-899).  Every other array has one row per pair of the call: blocked_l,
 * blocked_r [npairs][cap] (mvpMapPoints[i2] / [i2 + Nleft] holds a MapPoint with Observations() > 0, :2565-2567 / :2643-2645; NULL =
 * none), dir [npairs] (0 / 1 = bForward / 2 = bBackward, other values read as 0, NULL = all 0; the same level band for both cameras,
 * :2544-2549 / :2628-2633), and the queries as in orbm_search_by_projection_frame_batch_async without invzc and uright -- there is no
 * stereo gate when Nleft != -1 (:2569).  (u, v) is the left projection and (ur, vr) the projection of Trl * x3Dc into the right camera
 * (:2616-2618); they stay with the caller, must be finite, and valid folds the caller-side tests of :2505-2528, which test the LEFT
 * projection only -- a right window wholly outside the grid is simply empty (Frame.cc:802-824).  A query that is not valid, or whose
 * octave lies outside [0, nlevels), reads nothing else of its row.  Per valid query, in query order, exactly as
 * orbm_search_by_projection_frame_fisheye: radius th * scale[octave] (:2535, :2624) for both cameras; a left window without any
 * candidate finishes the query, the right block included (the `continue` of :2551; candidates are counted before blocked slots are
 * looked at); else the first candidate of least distance whose slot is not in the left blocked set is accepted at bestDist <= TH_HIGH
 * (:2556-2593), written to match_l and counted -- a later claim may overwrite the slot and counts again, and only mp_obs blocks the
 * slot for later queries --; then the same against the right row with its own blocked set, written to match_r (:2637-2661): a query
 * may claim one slot in each camera.  check_orientation: ONE 30-bin histogram with factor 30 / 360.0f (:2480) takes both cameras'
 * claims, the current keypoint's angle from the row that was claimed (:2602-2612, :2668-2677); ComputeThreeMaxima culls entries in
 * either row to ORBM_MATCH_PRUNED and each culled entry counts down once (:2688-2708), a slot claimed twice sitting in it twice.
 * retry_below > 0: a pair whose count is below it is searched again at 2 * th with both blocked sets empty (Tracking.cc:3213-3221);
 * that result replaces both rows and the count and retried[p] = 1 (retried [npairs] or NULL; 0 for the other pairs).  Outputs
 * (device): match_l, match_r [npairs][cap] (match_l[k] -> mvpMapPoints[k], match_r[k] -> mvpMapPoints[Nleft + k]; padded with
 * ORBM_NO_MATCH; a pair whose left row is empty gets two all-ORBM_NO_MATCH rows and 0), nmatches [npairs].  All pointers are device
 * pointers except scale_factors_host.  Enqueue-only: the scratch is the handle's grow-only one, so after one eager call the same or a
 * smaller shape allocates nothing and can be captured (orbx_capture_begin).  ORBM_E_INVALID: a NULL required array (blocked_l,
 * blocked_r, dir and retried may be NULL), a count < 1, first_l, first_r or retry_below < 0; ORBM_E_CAPACITY: cap > 65535, q_stride >
 * ORBM_LP_MAX_QUERIES, nlevels > 12, npairs > 65535.  Nothing is enqueued then. */
int orbm_search_by_projection_frame_fisheye_batch_async(orbm_t*, const orbm_kp_t* kps, const uint8_t* desc, const int32_t* counts, int cap,
                                                        const int32_t* grid_start, const int32_t* grid_idx,
                                                        float min_x, float min_y, float inv_w, float inv_h,
                                                        int first_l, int first_r, int npairs,
                                                        const uint8_t* blocked_l, const uint8_t* blocked_r, const uint8_t* dir,
                                                        const int32_t* nq, int q_stride, const uint8_t* valid,
                                                        const float* u, const float* v, const float* ur, const float* vr,
                                                        const int32_t* octave, const float* angle, const uint8_t* qdesc, const uint8_t* mp_obs,
                                                        float th, int retry_below, const float* scale_factors_host, int nlevels, int check_orientation,
                                                        int32_t* match_l, int32_t* match_r, int32_t* nmatches, uint8_t* retried);
/* orbm_search_by_projection_points_fisheye_batch_async: M3 SearchByProjection(Frame, vector<MapPoint*>, th, bFarPoints, thFarPoints) with
 * F.Nleft != -1 -- Tracking::SearchLocalPoints on a fisheye stereo rig -- END TO END on the device for `npairs` pairs
 * (ORBmatcher.cc:45-239, the right-camera block :170-236 and the mvLeftToRightMatch / mvRightToLeftMatch cross writes included); the
 * device form of orbm_search_by_projection_points_fisheye.  Pool and grid are those of
 * orbm_search_by_projection_frame_fisheye_batch_async: one pool of rows of `cap` slots with the grid of orbm_grid_build_batch_async
 * over it, pair p searches left row first_l+p and right row first_r+p.  Every other array has one row per pair of the call:
 * blocked_l, blocked_r [npairs][cap] (mvpMapPoints[idx] / [idx + Nleft] holds a MapPoint with Observations() > 0, :102-104 /
 * :194-196; NULL = none), l2r, r2l [npairs][cap] int32 (mvLeftToRightMatch / mvRightToLeftMatch: -1 or the partner slot; NULL = all
 * -1), and the queries: nq [npairs] local map points per pair in rows of q_stride entries -- in_view, proj_x, proj_y, view_cos, level
 * (mbTrackInView, mTrackProjX, mTrackProjY, mTrackViewCos, mnTrackScaleLevel) and in_view_r, proj_xr, proj_yr, view_cos_r, level_r
 * (the ...R fields); the frustum test of a KannalaBrandt8 camera stays with the caller.  depth [npairs][q_stride] (mTrackDepth; NULL
 * = bFarPoints off) with th_far; qdesc [..][32] and mp_obs [..] (Observations() > 0) are per pair rows too, or ONE row shared by
 * every pair when q_shared != 0.  Per pair, in query order, exactly as orbm_search_by_projection_points_fisheye:
 *   1. a query with neither in_view nor in_view_r, or with depth > th_far, is skipped (:56-60); a skipped query, or a skipped camera
 *      block, reads nothing else of its row;
 *   2. the left block (:65-168) runs when in_view is set and level lies in [0, nlevels): radius RadiusByViewingCos(view_cos) [* th if
 *      th != 1] * scale[level], levels [level-1, level], no stereo gate (:107), best / second over the candidates whose slot is not in
 *      the left blocked set by `dist < bestDist` / `else if dist < bestDist2` with the level of each (:125-141);
 *   3. a left claim needs bestDist <= TH_HIGH (:147) and passes when the levels differ or bestDist <= nnratio * bestDist2 (:154): it
 *      writes match_l[best] and counts 1, and if l2r[best] != -1 it also writes match_r[l2r[best]] and counts 1 more (:157-161); the
 *      cross write does not look at the blocked set and overwrites whatever that slot holds;
 *   4. a same-level ratio rejection in the left block is the `continue` of :151-152: it ends the query, right block included; an
 *      empty left window (:85), a left best above TH_HIGH and a left window whose candidates are all blocked do not, the right block
 *      still runs after them;
 *   5. the right block (:170-236) runs when in_view_r is set and level_r lies in [0, nlevels) (level_r == -1 is the reference's own
 *      skip, :172): radius RadiusByViewingCos(view_cos_r) * scale[level_r] with NO th factor (:173-176), the same best / second and
 *      ratio rules (:203-222) against the right blocked set; a claim first writes match_l[r2l[best]] if that is not -1 and counts 1,
 *      then writes match_r[best] and counts 1 (:224-233);
 *   6. only a query with mp_obs blocks the slots it wrote -- the cross-written ones too, in the other camera's blocked set -- for
 *      later searches; the right block of the same query already sees what its left block blocked; a later write may overwrite an
 *      unblocked slot and counts again;
 *   7. l2r[k] is honoured only where 0 <= l2r[k] < counts[right row], r2l[k] only where 0 <= r2l[k] < counts[left row]; any other
 *      value reads as -1 (nothing is written outside a row);
 *   8. an empty left row does not empty the pair: the right block still runs (unlike M4's :2551).
 * Outputs (device): match_l, match_r [npairs][cap] = query index or ORBM_NO_MATCH, padded to cap (match_l[k] -> mvpMapPoints[k],
 * match_r[k] -> mvpMapPoints[Nleft + k]); nmatches [npairs] = the return value of orbm_search_by_projection_points_fisheye.  All
 * pointers are device pointers except scale_factors_host.  Enqueue-only: the scratch is the handle's grow-only one, so after one
 * eager call the same or a smaller shape allocates nothing and can be captured (orbx_capture_begin).  ORBM_E_INVALID: a NULL handle
 * (checked first), a NULL required array (blocked_l, blocked_r, l2r, r2l and depth may be NULL), a count < 1, first_l or first_r < 0;
 * ORBM_E_CAPACITY: cap > 65535, q_stride > ORBM_LP_MAX_QUERIES, nlevels > 12, npairs > 65535.  Nothing is enqueued then. */
int orbm_search_by_projection_points_fisheye_batch_async(orbm_t*, const orbm_kp_t* kps, const uint8_t* desc, const int32_t* counts, int cap,
                                                         const int32_t* grid_start, const int32_t* grid_idx,
                                                         float min_x, float min_y, float inv_w, float inv_h,
                                                         int first_l, int first_r, int npairs,
                                                         const uint8_t* blocked_l, const uint8_t* blocked_r, const int32_t* l2r, const int32_t* r2l,
                                                         const int32_t* nq, int q_stride,
                                                         const uint8_t* in_view, const float* proj_x, const float* proj_y,
                                                         const float* view_cos, const int32_t* level,
                                                         const uint8_t* in_view_r, const float* proj_xr, const float* proj_yr,
                                                         const float* view_cos_r, const int32_t* level_r,
                                                         const float* depth, float th_far, const uint8_t* qdesc, const uint8_t* mp_obs, int q_shared,
                                                         float th, float nnratio, const float* scale_factors_host, int nlevels,
                                                         int32_t* match_l, int32_t* match_r, int32_t* nmatches);
/* orbm_project_last_frame_batch_async: the projection half of M4 (ORBmatcher.cc:2481-2527) for a pinhole camera with Nleft == -1, the
 * producer of the rows above.  Per pair (device): tcw_cur, tcw_last [npairs][12] (row-major 3x4 [R | t]); per query (device): x3dw
 * [npairs][q_stride][3] (world position), has_mp [npairs][q_stride] (pMP && !mvbOutlier), nq [npairs].  Host: k_host = (fx, fy, cx, cy),
 * bounds_host = (minX, maxX, minY, maxY), mb, mono.  Outputs (device): valid, u, v, invzc [npairs][q_stride] (rows beyond nq[p] are
 * not written; a rejected query gets valid = 0 and u = v = invzc = 0) and dir [npairs] (1 = bForward, 2 = bBackward, else 0).
 * Numerics are those of the facade against cvcompat.h: x3Dc = (float)(double sum of R * X) + t, invzc = (float)(1.0 / (double)z),
 * u = fx * xc / zc + cx in float without contraction; twc = -Rcw^T * tcw and tlc = Rlw * twc + tlw by the same product rule.  A point
 * with z == 0 exactly is outside the contract.  Enqueue-only; ORBM_E_INVALID: a NULL array, npairs or q_stride < 1; ORBM_E_CAPACITY:
 * q_stride > ORBM_LP_MAX_QUERIES, npairs > 65535. */
int orbm_project_last_frame_batch_async(orbm_t*, int npairs, const float* tcw_cur, const float* tcw_last, const int32_t* nq, int q_stride,
                                        const float* x3dw, const uint8_t* has_mp, const float* k_host, const float* bounds_host, float mb, int mono,
                                        uint8_t* valid, float* u, float* v, float* invzc, uint8_t* dir);
/* orbm_fuse_batch_async: M13 Fuse(pKF, vpMapPoints, th) -- LocalMapping::SearchInNeighbors (LocalMapping.cc:925-1070) -- and its Sim3 twin
 * Fuse(pKF, Scw, vpPoints, th, vpReplacePoint) -- LoopClosing::SearchAndFuse -- search core END TO END on the device for `npairs` (KeyFrame
 * row, query row) pairs (ORBmatcher.cc:1823-2049 with chi2_gate = 1, :2051-2199 with chi2_gate = 0), pinhole camera, Nleft == -1; the
 * bRight / fisheye call stays with orbm_fuse.  The KeyFrame pool has nkf_rows rows of cap slots: kps_kf (mvKeysUn), desc_kf [..][32],
 * uright_kf (mvuRight; NULL = every slot < 0) and the grid of orbm_grid_build_batch_async over the pool, indexed by row -- the grid is how
 * the search reaches a slot.  An extractor result block is one valid pool, a caller-gathered array of KeyFrame rows another.  Pair p reads
 * KF row kf_row[p] (NULL = row p); tcw [npairs][12] is its row-major 3x4 [Rcw | tcw] and ow [npairs][3] its camera centre: GetRotation /
 * GetTranslation / GetCameraCenter for chi2_gate = 1, or Rcw = sRcw / scw, tcw / scw and Ow = -Rcw^T tcw as the caller computes them for
 * the Sim3 variant.  The queries are MapPoints: nq [npairs] of them per pair; valid [npairs][q_stride] holds the caller-side tests (pMP &&
 * !isBad(), plus !IsInKeyFrame(pKF) or !spAlreadyFound.count(pMP)); pw [..][3] (GetWorldPos), normal [..][3] (GetNormal), min_dist /
 * max_dist (mfMinDistance / mfMaxDistance) and qdesc [..][32] are rows of q_stride entries per pair, or ONE row shared by every pair when
 * q_shared != 0.  A query that is not valid reads nothing else.  Numerics are those of the facade's Fuse lines against cvcompat.h: x3Dc =
 * (float)(double sum of R * X) + t, z < 0 rejects, invz = 1 / z, u = fx * x / z + cx in float without contraction, IsInImage (u >= minX
 * && u < maxX && v >= minY && v < maxY; k_host = (fx, fy, cx, cy), bounds_host = (minX, maxX, minY, maxY)), ur = u - bf * invz, dist3D =
 * (float)sqrt(double sum of PO^2) within [0.8f * min_dist, 1.2f * max_dist], PO . normal (double) >= 0.5 * dist3D, PredictScale as
 * orbm_is_in_frustum computes it (log_scale_factor, nlevels); a point with z == 0 exactly is outside the contract.  The window is
 * KeyFrame::GetFeaturesInArea(u, v, th * scale[level]) without a stereo gate; candidates of levels [level-1, level]; chi2_gate adds the
 * test e2 * inv_sigma2[octave] > 7.8 (with er = ur - uright[k] where uright[k] >= 0) or > 5.99 (two terms); the first minimum in visiting
 * order is accepted at bestDist <= TH_LOW.  Outputs (device): best_idx [npairs][q_stride] = KF slot or -1 (the row orbm_fuse returns,
 * padded with -1 to q_stride), nfused [npairs] = its return value, level_out [npairs][q_stride] (NULL = not written) = the predicted
 * level of a query that passed every geometric gate, else -1.  A pair whose kf_row lies outside [0, nkf_rows) gets an all -1 row and 0.
 * AddObservation / Replace stay with the caller (the cross-KeyFrame rule).  All pointers are device pointers except
 * the *_host tables; enqueue-only, no scratch: every call can be captured (orbx_capture_begin) after one eager call.  ORBM_E_INVALID: a
 * NULL required array (inv_sigma2_host only with chi2_gate), npairs, nkf_rows, cap, q_stride or nlevels < 1, th not finite;
 * ORBM_E_CAPACITY: cap > 65535, q_stride > ORBM_LP_MAX_QUERIES, nlevels > 12, npairs > 65535.  Nothing is enqueued then. */
int orbm_fuse_batch_async(orbm_t*, int npairs,
                          int nkf_rows, int cap, const orbm_kp_t* kps_kf, const uint8_t* desc_kf, const float* uright_kf,
                          const int32_t* grid_start, const int32_t* grid_idx, float min_x, float min_y, float inv_w, float inv_h,
                          const int32_t* kf_row, const float* tcw, const float* ow,
                          const int32_t* nq, int q_stride, const uint8_t* valid,
                          const float* pw, const float* normal, const float* min_dist, const float* max_dist, const uint8_t* qdesc, int q_shared,
                          const float* k_host, const float* bounds_host, float bf,
                          float th, int chi2_gate, const float* scale_factors_host, const float* inv_sigma2_host,
                          float log_scale_factor, int nlevels,
                          int32_t* best_idx, int32_t* nfused, int32_t* level_out);
/* orbm_search_by_projection_kf_batch_async: M5 SearchByProjection(Frame&, KeyFrame*, sAlreadyFound, th, ORBdist) -- the two guided
 * searches of Tracking::Relocalization (Tracking.cc:4309 with th 10 / ORBdist 100, :4334 with th 3 / ORBdist 64) -- END TO END on the
 * device for `npairs` (frame row, candidate KeyFrame, pose) triples (ORBmatcher.cc:2723-2852), pinhole camera, Nleft == -1; the fisheye
 * call stays with orbm_search_by_projection_kf.  The frame pool has nf_rows rows of cap slots: kps_f (mvKeysUn), desc_f [..][32],
 * counts_f and the grid of orbm_grid_build_batch_async over the pool, indexed by row.  Pair p searches row f_row[p] (NULL = row p): one
 * frame against N relocalisation candidates repeats the row.  f_blocked [npairs][cap] = CurrentFrame.mvpMapPoints[i2] != NULL in this
 * candidate's state (NULL = none blocked); tcw [npairs][12] is the candidate's pose (mCurrentFrame.mTcw after PnP / PoseOptimization)
 * as a row-major 3x4 [Rcw | tcw], ow [npairs][3] = -Rcw^T tcw as the caller computes it.  Query i of pair p is KeyFrame slot i
 * (pKF->GetMapPointMatches()[i]); nq [npairs] of them in rows of q_stride: valid (pMP && !isBad() && !sAlreadyFound.count(pMP)),
 * pw [..][3] (GetWorldPos), min_dist / max_dist (mfMinDistance / mfMaxDistance), angle (pKF->mvKeysUn[i].angle) and qdesc [..][32]
 * (GetDescriptor).  A query that is not valid reads nothing else.  Numerics are those of the facade's M5 lines against cvcompat.h:
 * x3Dc = (float)(double sum of R * X) + t, u = fx * x / z + cx in float without contraction and NO depth test, closed bounds (reject
 * only u < minX || u > maxX || v < minY || v > maxY; k_host = (fx, fy, cx, cy), bounds_host = (minX, maxX, minY, maxY)), dist3D =
 * (float)sqrt(double sum of PO^2) within [0.8f * min_dist, 1.2f * max_dist], PredictScale as orbm_is_in_frustum computes it
 * (log_scale_factor, nlevels of the frame); a point with z == 0 exactly is outside the contract.  The window is
 * Frame::GetFeaturesInArea(u, v, th * scale[level], level - 1, level + 1) without a stereo gate.  Claims run in query order: the first
 * candidate of least distance whose slot is not blocked is accepted at bestDist <= orb_dist and EVERY claim blocks its slot
 * (:2791-2793); with check_orientation the 30-bin histogram of angle_kf - angle_f and the three-maxima cull follow.  Outputs (device):
 * match [npairs][cap] = the row orbm_search_by_projection_kf returns (query index / ORBM_NO_MATCH / ORBM_MATCH_PRUNED, padded with
 * ORBM_NO_MATCH to cap), nmatches [npairs] = its return value.  A pair whose f_row lies outside [0, nf_rows) gets an all
 * ORBM_NO_MATCH row and 0.  All pointers are device pointers except the *_host tables; enqueue-only: the handle's work buffers are
 * allocated by the first eager call and reused, so after one eager call of the same or a smaller shape the call can be captured
 * (orbx_capture_begin) and allocates nothing.  ORBM_E_INVALID: a NULL required array, npairs, nf_rows, cap, q_stride or nlevels < 1,
 * th not finite, orb_dist > 255 (a negative orb_dist matches nothing); ORBM_E_CAPACITY: cap > 65535, q_stride > ORBM_LP_MAX_QUERIES,
 * nlevels > 12, npairs > 65535.  Nothing is enqueued then. */
int orbm_search_by_projection_kf_batch_async(orbm_t*, int npairs,
                                             int nf_rows, int cap, const orbm_kp_t* kps_f, const uint8_t* desc_f, const int32_t* counts_f,
                                             const int32_t* grid_start, const int32_t* grid_idx, float min_x, float min_y, float inv_w, float inv_h,
                                             const int32_t* f_row, const uint8_t* f_blocked, const float* tcw, const float* ow,
                                             const int32_t* nq, int q_stride, const uint8_t* valid, const float* pw,
                                             const float* min_dist, const float* max_dist, const float* angle, const uint8_t* qdesc,
                                             const float* k_host, const float* bounds_host, float th, int orb_dist,
                                             const float* scale_factors_host, float log_scale_factor, int nlevels, int check_orientation,
                                             int32_t* match, int32_t* nmatches);

/* ---- batched, DEVICE-resident stereo step (config C3: EuRoC stereo).  All pointers are device pointers; enqueue only.
 * orbm_stereo_batch_async: M15 Frame::ComputeStereoMatches (Frame.cc:1027-1276) for `npairs` stereo pairs of ONE extractor
 * batch: pair p = frames (first_l + p, first_r + p); kps / desc / counts = that extractor's result block (orbx_result_device),
 * cap = orbx_max_keypoints.  The row-band candidates, Hamming, SAD slide and parabola run per left keypoint on the
 * device-resident pyramids; the median cut (:1261-1275) is a second kernel.  Outputs [npairs][cap]: uright (mvuRight), depth
 * (mvDepth), sad (scratch: best SAD or -1); kept[npairs] = stereo points that survive the cut.
 * orbm_bow_nodes_batch_async: Frame::ComputeBoW's FeatureVector bucket of every descriptor row (8(f).1 tree descent, node at
 * `levelsup` levels above the leaves) for nrows rows of a result block: node_id[nrows].
 * orbm_triangulation_batch_async: M10 SearchForTriangulation_ (ORBmatcher.cc:1388-1629; pinhole, no MapPoints attached, no
 * orientation check: how LocalMapping calls it, LocalMapping.cc:514-516,592) for `npairs` KeyFrame pairs: KeyFrame 1 of pair p
 * = row p of the *1 arrays ([npairs][cap] slices of a result block + its node ids and mvuRight), KeyFrame 2 likewise.  A
 * bucket = equal node id, walked in ascending index order as the FeatureVector is.  matches12 [npairs][cap] = idx2 or -1,
 * nmatches[npairs]. */
int orbm_stereo_batch_async(orbm_t*, void* extractor, int first_l, int first_r, int npairs, const orbm_kp_t* kps, const uint8_t* desc,
                            const int32_t* counts, int cap, float mb, float mbf, float* uright, float* depth, int32_t* sad, int32_t* kept);
int orbm_bow_nodes_batch_async(orbm_t*, const struct orbm_vocab* vocab, const uint8_t* desc, int nrows, int levelsup, int32_t* node_id);
int orbm_triangulation_batch_async(orbm_t*, int npairs, int cap,
                                   const orbm_kp_t* kps1, const uint8_t* desc1, const int32_t* counts1, const int32_t* node1, const float* uright1,
                                   const orbm_kp_t* kps2, const uint8_t* desc2, const int32_t* counts2, const int32_t* node2, const float* uright2,
                                   const float* F12, float epx, float epy, const float* scale_factors2, const float* level_sigma2_2, int nlevels,
                                   int only_stereo, int coarse, int32_t* matches12, int32_t* nmatches);

/* ---- DBoW2 vocabulary transform (Frame::ComputeBoW, Frame.cc:905-918;
 * Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1125-1262, FORB::distance FORB.cpp:81-101) ----
 * The tree lives in HBM; orbm_bow_transform descends it for n descriptors (host pointers) and returns per feature the
 * word id, the node id `levelsup` levels above the leaves (the SearchByBoW bucket) and the word weight (0 = stopped).
 * orbm_bow_vectors assembles BowVector (TF-IDF, L1-normalised: the ORBvoc configuration) and FeatureVector (CSR) on the
 * host exactly as the std::map based classes do.
 * The text header is `k L scoring weighting`.  The reference switches transform on the last two (:1145-1193: TF / TF_IDF add
 * weights, IDF / BINARY insert once; a scoring type that does not normalise divides by v.size()); orbm_bow_vectors implements
 * TF_IDF + L1 only, so orbm_vocab_load_text refuses every header whose scoring / weighting pair is not `0 0` with ORBM_E_INVALID
 * and a message that names the two fields.  A node may have at most 31 children (orbm_vocab_create; the text header's k is
 * at most 20, :1359). */
typedef struct orbm_vocab orbm_vocab_t;
int orbm_vocab_load_text(orbm_t*, orbm_vocab_t** out, const char* path);     /* loadFromTextFile, :1338-1440 */
int orbm_vocab_create(orbm_t*, orbm_vocab_t** out, int k, int L, int nnodes, const int32_t* parent, const uint8_t* is_leaf,
                      const uint8_t* desc, const double* weight);            /* node 0 = root; ids in file order */
void orbm_vocab_destroy(orbm_vocab_t*);
int orbm_vocab_info(const orbm_vocab_t*, int* k, int* L, int* nnodes, int* nwords);
int orbm_bow_transform(orbm_t*, const orbm_vocab_t*, const uint8_t* desc, int n, int levelsup,
                       int32_t* word_id, int32_t* node_id, double* weight);
int orbm_bow_vectors(int n, const int32_t* word_id, const int32_t* node_id, const double* weight,
                     int32_t* bow_ids, double* bow_vals, int* nbow,
                     int32_t* fv_nodes, int32_t* fv_start, int32_t* fv_idx, int* nfv);

/* orbm_bow_transform_batch_async: the device form of orbm_bow_transform for nrows descriptor rows (e.g. a whole result block,
 * [frames][cap] rows; slots beyond a frame's count give values nobody reads).  word_id, node_id, weight [nrows]; word_id and weight
 * may be NULL, node_id may not.  weight 0 marks a stopped word, which DBoW2 leaves out of the FeatureVector (TemplatedVocabulary.h:1157,
 * `w > 0`): orbm_search_by_bow_batch_async reads it for that rule.  All pointers are device pointers; enqueue-only (capturable).
 * ORBM_E_INVALID: a NULL handle, vocabulary, desc or node_id, nrows < 1, a vocabulary of another device. */
int orbm_bow_transform_batch_async(orbm_t*, const orbm_vocab_t* vocab, const uint8_t* desc, int nrows, int levelsup,
                                   int32_t* word_id, int32_t* node_id, double* weight);
/* orbm_search_by_bow_batch_async: M7 SearchByBoW(KeyFrame*, Frame&, vpMapPointMatches) -- Tracking::TrackReferenceKeyFrame
 * (Tracking.cc:3002-3015, nnratio 0.7) and Tracking::Relocalization (Tracking.cc:4175-4215, nnratio 0.75, one call per candidate
 * KeyFrame) -- END TO END on the device for `npairs` pairs (ORBmatcher.cc:314-547, the Nleft == -1 part; the fisheye / right-camera
 * branch :406-433, :471-498 is orbm_search_by_bow_fisheye_batch_async below).  Two pools of rows: the KeyFrame pool has nkf_rows rows of cap_kf
 * slots -- kps_kf (mvKeysUn), desc_kf [..][32], counts_kf [nkf_rows], node_kf / weight_kf (orbm_bow_transform_batch_async over the
 * rows), good_kf (pMP && !pMP->isBad()) --, the frame pool nf_rows rows of cap_f slots with the same arrays but good.  An extractor
 * result block is one valid pool, a caller-gathered array of KeyFrame rows in the same layout another.  Pair p matches KF row kf_row[p]
 * against frame row f_row[p] (NULL = row p): P frames against their reference KeyFrames, or one frame against N relocalization
 * candidates (f_row all equal).  Per pair the FeatureVector buckets are the features of one node id in ascending index, without the
 * stopped words (weight <= 0; NULL weight = none), without KF features whose good_kf is 0 and without slots >= count.  Per KF feature
 * in bucket order: the first minimum over the bucket's unmatched frame features, bestDist1 <= TH_LOW and bestDist1 < nnratio *
 * bestDist2 (the if / else-if runner-up) claim the frame feature; check_orientation applies the 30-bin rotation histogram (rot =
 * angle_kf - angle_f) and its three-maxima cull.  Outputs (device): f_match [npairs][cap_f] = KF feature index or -1 (culled matches
 * -1 too: the row orbm_search_by_bow returns, padded with -1 to cap_f), nmatches [npairs] = its return value.  A pair whose kf_row or
 * f_row lies outside [0, nkf_rows) / [0, nf_rows) gets an all -1 row and 0.  The TrackReferenceKeyFrame / Relocalization tests on
 * nmatches (< 15) stay with the caller.  All pointers are device pointers; enqueue-only, no scratch: every call can be captured
 * (orbx_capture_begin) once one eager call with the same or a larger cap_kf / cap_f has run.  ORBM_E_INVALID: a NULL required array,
 * npairs, nkf_rows, nf_rows, cap_kf or cap_f < 1, nnratio not finite; ORBM_E_CAPACITY: cap_kf or cap_f > ORBM_BOW_MAX_CAP (the bucket
 * lists and the pair's row live in LDS), npairs > 65535.  Nothing is enqueued then. */
enum { ORBM_BOW_MAX_CAP = 24576 };
int orbm_search_by_bow_batch_async(orbm_t*, int npairs,
                                   int nkf_rows, int cap_kf, const orbm_kp_t* kps_kf, const uint8_t* desc_kf, const int32_t* counts_kf,
                                   const int32_t* node_kf, const double* weight_kf, const uint8_t* good_kf,
                                   int nf_rows, int cap_f, const orbm_kp_t* kps_f, const uint8_t* desc_f, const int32_t* counts_f,
                                   const int32_t* node_f, const double* weight_f,
                                   const int32_t* kf_row, const int32_t* f_row, float nnratio, int check_orientation,
                                   int32_t* f_match, int32_t* nmatches);
/* orbm_search_by_bow_fisheye_batch_async: M7 SearchByBoW(KeyFrame*, Frame&, vpMapPointMatches) with F.Nleft != -1 (a two-camera rig:
 * ORBmatcher.cc:343-545 with the else branch of :406-433 and the nested acceptance of :438-500) -- Tracking::TrackReferenceKeyFrame
 * (Tracking.cc:3006) and one call per candidate KeyFrame of Tracking::Relocalization (Tracking.cc:4201) -- END TO END on the device for
 * `npairs` pairs; the device form of orbm_search_by_bow_fisheye.  The KeyFrame pool is exactly that of orbm_search_by_bow_batch_async
 * (nkf_rows rows of cap_kf slots, kf_row[p], NULL = row p); a two-camera KeyFrame is ONE stacked row, left features then right, as
 * pKF->mDescriptors and vpMapPointsKF are stacked, and the caller puts the mvKeys / mvKeysRight angles into kps_kf (only `angle` is
 * read, :447-450).  The frame pool has nf_rows rows of cap_f slots (kps_f, desc_f, counts_f, node_f, weight_f: an extractor result block
 * and orbm_bow_transform_batch_async over its rows).  The three differences from orbm_search_by_bow_batch_async:
 *  1. Two frame rows per pair.  Pair p uses left row fl_row[p] (mvKeys) and right row fr_row[p] (mvKeysRight); both arrays are required
 *     (one lost frame meets N relocalization candidates by repeating its two rows).  realIdxF is j for left slot j and Nleft + j for
 *     right slot j, Nleft = counts_f[fl_row[p]]: a bucket is walked left entries first, then right, each in ascending slot.
 *  2. The nested acceptance.  Per KeyFrame feature in bucket order, over the bucket's unclaimed frame features of the same node, the left
 *     candidates give bestDist1 / bestIdxF / bestDist2 and the right ones bestDist1R / bestIdxFR (first minimum in index order, the
 *     if / else-if runner-up).  The left slot is claimed iff bestDist1 <= TH_LOW and (float)bestDist1 < nnratio * (float)bestDist2.  The
 *     right slot is claimed iff bestDist1 <= TH_LOW (the LEFT distance) and bestDist1R <= TH_LOW: its ratio test is switched off by
 *     `|| true` (:473), it does not wait for the left ratio test to pass, and it never happens where the node holds no unclaimed left
 *     candidate.  A claimed slot of either camera is skipped by later KeyFrame features (:409).
 *  3. Two output rows and ONE histogram.  check_orientation fills one 30-bin histogram with both cameras' claims (rot = angle_kf - angle
 *     of the claimed row's keypoint, factor 30/360.0f, round, bin 30 -> 0); after the three-maxima cull an entry of another bin becomes
 *     -1 in the row that holds it and counts down once.  Outputs (device): f_match_l, f_match_r [npairs][cap_f] = KeyFrame feature index
 *     or -1, padded with -1; nmatches [npairs] = the return value of orbm_search_by_bow_fisheye.
 * Stopped words (weight <= 0; NULL weight = none), KeyFrame features with good_kf == 0 and slots >= count are left out as in M7.  A pair
 * whose kf_row, fl_row or fr_row is out of range gets two all -1 rows and 0.  The bucket lists and the claimed row run over both cameras
 * in LDS as ushorts: 2 * cap_kf + 8 * cap_f + 10408 bytes <= 160 KB, published as cap_f <= ORBM_BOW_FISHEYE_MAX_CAP_F PER CAMERA with
 * cap_kf <= ORBM_BOW_MAX_CAP (157864 bytes, the footprint of M7 at its own cap).  All pointers are device pointers; enqueue-only, no
 * scratch: every call can be captured (orbx_capture_begin) once one eager call with the same or larger caps has run.  ORBM_E_INVALID: a
 * NULL required array (kf_row and the weights may be NULL), npairs, nkf_rows, nf_rows, cap_kf or cap_f < 1, nnratio not finite;
 * ORBM_E_CAPACITY: cap_kf > ORBM_BOW_MAX_CAP, cap_f > ORBM_BOW_FISHEYE_MAX_CAP_F, npairs > 65535.  Every check runs before the device is
 * touched; nothing is enqueued then. */
enum { ORBM_BOW_FISHEYE_MAX_CAP_F = 12288 };
int orbm_search_by_bow_fisheye_batch_async(orbm_t*, int npairs,
                                           int nkf_rows, int cap_kf, const orbm_kp_t* kps_kf, const uint8_t* desc_kf, const int32_t* counts_kf,
                                           const int32_t* node_kf, const double* weight_kf, const uint8_t* good_kf,
                                           int nf_rows, int cap_f, const orbm_kp_t* kps_f, const uint8_t* desc_f, const int32_t* counts_f,
                                           const int32_t* node_f, const double* weight_f,
                                           const int32_t* kf_row, const int32_t* fl_row, const int32_t* fr_row, float nnratio, int check_orientation,
                                           int32_t* f_match_l, int32_t* f_match_r, int32_t* nmatches);
/* orbm_search_by_bow_kf_batch_async: M8 SearchByBoW(KeyFrame* pKF1, KeyFrame* pKF2, vpMatches12) -- LoopClosing::DetectCommonRegionsFromBoW
 * (LoopClosing.cc:822, matcher(0.9, true): the current KeyFrame against every candidate and its covisibles) -- END TO END on the device for
 * `npairs` pairs (ORBmatcher.cc:955-1105, Nleft == -1; fisheye KeyFrames stay with orbm_search_by_bow_kf).  Two pools of rows as in
 * orbm_search_by_bow_batch_async: pool 1 has nrows1 rows of cap1 slots -- kps1 (mvKeysUn), desc1 [..][32], counts1 [nrows1], node1 / weight1
 * (orbm_bow_transform_batch_async over the rows), good1 (pMP && !pMP->isBad()) --, pool 2 the same arrays with nrows2 / cap2; a caller with
 * one pool passes it twice.  Pair p matches row row1[p] of pool 1 (pKF1) against row row2[p] of pool 2 (pKF2); NULL = row p; place
 * recognition repeats row1.  Where M8 differs from M7: BOTH sides drop features without a good MapPoint (:1000-1004, :1021-1028) besides
 * the stopped words (weight <= 0; NULL weight = none) and slots >= count; the outer loop is pKF1's bucket in ascending feature index and
 * the claimed side is pKF2 (vbMatched2); bestDist1 < TH_LOW is STRICT (:1054; M7 has <=) with (float)bestDist1 < nnratio *
 * (float)bestDist2 and the if / else-if runner-up; check_orientation: rot = angle1 - angle2, factor 30/360.0f, round, bin 30 -> 0, the
 * three-maxima cull; a culled idx1 becomes -1 and is not counted.  Outputs (device): matches12 [npairs][cap1] = the pKF2 feature index of
 * pKF1 feature idx1, or -1 (the row orbm_search_by_bow_kf returns, padded with -1 to cap1), nmatches [npairs] = its return value.  A pair
 * whose row1 or row2 lies outside [0, nrows1) / [0, nrows2) gets an all -1 row and 0.  The kernel is M7's (one workgroup per pair, bucket
 * lists and the claimed-side row over cap2 in LDS); M7 at ORBM_BOW_MAX_CAP already uses 157 of the 160 KB, so there is no second LDS row
 * over cap1: the claimed-side row is transposed into matches12 at the end (fill -1, barrier, scatter), and ORBM_BOW_MAX_CAP holds for both
 * caps here too.  All pointers are device pointers; enqueue-only, no scratch: every call can be captured (orbx_capture_begin) once one
 * eager call with the same or larger caps has run.  ORBM_E_INVALID: a NULL required array (the weights may be NULL), npairs, nrows1,
 * nrows2, cap1 or cap2 < 1, nnratio not finite; ORBM_E_CAPACITY: cap1 or cap2 > ORBM_BOW_MAX_CAP, npairs > 65535.  Nothing is enqueued
 * then. */
int orbm_search_by_bow_kf_batch_async(orbm_t*, int npairs,
                                      int nrows1, int cap1, const orbm_kp_t* kps1, const uint8_t* desc1, const int32_t* counts1,
                                      const int32_t* node1, const double* weight1, const uint8_t* good1,
                                      int nrows2, int cap2, const orbm_kp_t* kps2, const uint8_t* desc2, const int32_t* counts2,
                                      const int32_t* node2, const double* weight2, const uint8_t* good2,
                                      const int32_t* row1, const int32_t* row2, float nnratio, int check_orientation,
                                      int32_t* matches12, int32_t* nmatches);
/* orbm_search_by_projection_sim3_batch_async: M6 SearchByProjection(pKF, Scw, vpPoints, vpMatched, th, ratioHamming) (ORBmatcher.cc:549-679)
 * and its vpPointsKFs overload (:681-797) -- LoopClosing::DetectCommonRegionsFromBoW (LoopClosing.cc:963 with th 8 / ratio 1.5, :993 with
 * 5 / 1.0) and FindMatchesByProjection (:1248, 3 / 1.5) -- END TO END on the device for `npairs` (KeyFrame row, Sim3 pose, MapPoint row)
 * triples, pinhole camera, Nleft == -1; fisheye KeyFrames and other cameras stay with orbm_search_by_projection_sim3.  The KeyFrame pool
 * has nkf_rows rows of cap slots: kps_kf (mvKeysUn), desc_kf [..][32], counts_kf and the grid of orbm_grid_build_batch_async over the pool,
 * indexed by row.  Pair p searches row kf_row[p] (NULL = row p); tcw [npairs][12] is the row-major 3x4 [Rcw | tcw] with Rcw = sRcw / scw
 * and tcw / scw, ow [npairs][3] = -Rcw^T tcw, as the caller computes them from Scw; matched_in [npairs][cap] = vpMatched[idx] != NULL
 * (NULL = none).  The queries are MapPoints: nq [npairs] of them per pair in rows of q_stride: valid (!pMP->isBad() &&
 * !spAlreadyFound.count(pMP)), pw [..][3] (GetWorldPos), normal [..][3] (GetNormal), min_dist / max_dist (mfMinDistance / mfMaxDistance),
 * qdesc [..][32] (GetDescriptor).  A query that is not valid reads nothing else.  Projection and gates are those of orbm_fuse_batch_async
 * (x3Dc = (float)(double sum of R * X) + t, z < 0 rejects, half-open IsInImage, [0.8f * min_dist, 1.2f * max_dist], PO . normal < 0.5 *
 * dist rejects, PredictScale with log_scale_factor / nlevels) with ONE difference that proj_form selects: 0 = mpCamera->project, u = fx *
 * x / z + cx (:602); 1 = the vpPointsKFs overload's invz = 1 / z, u = fx * (x * invz) + cx (:724-729).  They round differently.  The window
 * is KeyFrame::GetFeaturesInArea(u, v, th * scale[level]); candidates of levels [level-1, level]; slots with matched set are skipped; the
 * first minimum in visiting order is accepted when (float)bestDist <= TH_LOW * ratio_hamming (the float product, as the reference writes
 * it).  Claims run in query order and EVERY claim blocks its slot for later queries; no rotation check.  A window whose candidates are all
 * blocked leaves bestDist = 256, where the reference would write vpMatched[-1] if the bound reached it: a ratio_hamming with
 * 50 * ratio_hamming >= 256 is refused.  Outputs (device): match [npairs][cap] = the query index iMP assigned to KeyFrame slot idx, or -1
 * (the row orbm_search_by_projection_sim3 returns, padded with -1 to cap), nmatches [npairs] = its return value.  A pair whose kf_row lies
 * outside [0, nkf_rows) gets an all -1 row and 0.  All pointers are device pointers except the *_host tables; enqueue-only: the handle's
 * work buffers are allocated by the first eager call and reused, so after one eager call of the same or a smaller shape the call can be
 * captured (orbx_capture_begin) and allocates nothing.  ORBM_E_INVALID: a NULL required array, npairs, nkf_rows, cap, q_stride or nlevels
 * < 1, ratio_hamming not finite or 50 * ratio_hamming >= 256, proj_form not 0 / 1; ORBM_E_CAPACITY: cap > 65535, q_stride >
 * ORBM_LP_MAX_QUERIES, nlevels > 12, npairs > 65535.  Nothing is enqueued then. */
int orbm_search_by_projection_sim3_batch_async(orbm_t*, int npairs,
                                               int nkf_rows, int cap, const orbm_kp_t* kps_kf, const uint8_t* desc_kf, const int32_t* counts_kf,
                                               const int32_t* grid_start, const int32_t* grid_idx, float min_x, float min_y, float inv_w, float inv_h,
                                               const int32_t* kf_row, const uint8_t* matched_in, const float* tcw, const float* ow,
                                               const int32_t* nq, int q_stride, const uint8_t* valid, const float* pw, const float* normal,
                                               const float* min_dist, const float* max_dist, const uint8_t* qdesc,
                                               const float* k_host, const float* bounds_host, int th, float ratio_hamming, int proj_form,
                                               const float* scale_factors_host, float log_scale_factor, int nlevels,
                                               int32_t* match, int32_t* nmatches);
/* orbm_search_for_triangulation_batch_async: M10 SearchForTriangulation_(pKF1, pKF2, vMatchedPairs, bOnlyStereo, bCoarse) --
 * LocalMapping::CreateNewMapPoints (LocalMapping.cc:492-495, 542-592: the new KeyFrame against its 10 / 20 best covisible neighbours) -- END
 * TO END on the device for `npairs` (pKF1 row, pKF2 row, F12, epipole) pairs (ORBmatcher.cc:1388-1629), pinhole cameras, Nleft == -1; the
 * second-camera and non-pinhole paths stay with orbm_search_for_triangulation_gated.  Two pools of rows as in
 * orbm_search_by_bow_kf_batch_async: pool 1 has nrows1 rows of cap1 slots -- kps1 (mvKeysUn), desc1 [..][32], counts1 [nrows1], node1 /
 * weight1 (orbm_bow_transform_batch_async over the rows; weight NULL = no stopped word), has_mp1 [nrows1][cap1] (GetMapPoint(idx) != NULL,
 * per ROW), uright1 [nrows1][cap1] (mvuRight; NULL = no stereo feature) --, pool 2 the same arrays with nrows2 / cap2; a caller with one
 * pool passes it twice.  Pair p matches row row1[p] of pool 1 (pKF1) against row row2[p] of pool 2 (pKF2); NULL = row p;
 * CreateNewMapPoints repeats row1.  Per pair geometry is device data the caller computes on the host as the facade's
 * SearchForTriangulation_ does: F12 [npairs][9] row-major, ep [npairs][2] = pKF2->mpCamera->project(R2w * Cw + t2w); a non-finite epipole
 * (sideways motion: z == 0) is legal and compares as IEEE does.  Semantics per pair are exactly those of orbm_search_for_triangulation: a
 * FeatureVector bucket is the features of one node id without the stopped words (weight <= 0), without slots >= count and without
 * features that have a MapPoint, on both sides; with only_stereo also without non-stereo features (uright < 0).  Per pKF1 feature: dist >
 * TH_LOW rejects (inclusive bound); where neither feature is stereo, distex^2 + distey^2 < 100 * scale_factors2[kp2.octave] rejects;
 * Pinhole::epipolarConstrain_ with den == 0 rejecting and dsqr < 3.84 * level_sigma2_2[kp2.octave] compared against the double product,
 * `coarse` accepts whatever it says; the survivor is the smallest distance among the gate-passing candidates and, on a tie, the LAST in
 * ascending idx2.  vbMatched2 is not kept by this overload (:1567): several idx1 may share an idx2, features are independent.
 * check_orientation: rot = angle1 - angle2 (+360 if negative), bin = round(rot * (1.0f / 30)) as written at :1441, bin 30 -> 0, then the
 * three-maxima cull; a culled idx1 becomes -1 and is not counted.  A pKF2 feature whose octave lies outside [0, nlevels) never matches: the
 * kernels do not index the level tables with it (the host entry point would).  Outputs (device): matches12 [npairs][cap1] = idx2 or -1
 * (the row orbm_search_for_triangulation returns, padded with -1 to cap1), nmatches [npairs] = its return value, computed from the
 * finished row (nothing accumulates across graph replays).  A pair whose row1 or row2 lies outside [0, nrows1) / [0, nrows2) gets an all
 * -1 row and 0.  The baseline / median-depth tests, the triangulation and AddMapPoint stay with the caller (the
 * cross-pair rule).  All pointers are device pointers except the *_host tables; enqueue-only: the handle's work buffers (the bucket lists per
 * pool-2 row) are allocated by the first eager call and reused, so after one eager call of the
 * same or a smaller shape the call can be captured (orbx_capture_begin) and allocates nothing.  ORBM_E_INVALID: a NULL required array
 * (the weights, urights and row arrays may be NULL), npairs, nrows1, nrows2, cap1, cap2 or nlevels < 1; ORBM_E_CAPACITY: cap1 or cap2 >
 * 65535 (16-bit bucket lists), nlevels > 12, npairs > 65535.  Nothing is enqueued then. */
int orbm_search_for_triangulation_batch_async(orbm_t*, int npairs,
                                              int nrows1, int cap1, const orbm_kp_t* kps1, const uint8_t* desc1, const int32_t* counts1,
                                              const int32_t* node1, const double* weight1, const uint8_t* has_mp1, const float* uright1,
                                              int nrows2, int cap2, const orbm_kp_t* kps2, const uint8_t* desc2, const int32_t* counts2,
                                              const int32_t* node2, const double* weight2, const uint8_t* has_mp2, const float* uright2,
                                              const int32_t* row1, const int32_t* row2, const float* F12, const float* ep,
                                              const float* scale_factors2_host, const float* level_sigma2_2_host, int nlevels,
                                              int only_stereo, int coarse, int check_orientation,
                                              int32_t* matches12, int32_t* nmatches);
/* orbm_search_for_initialization_batch_async: M9 SearchForInitialization(F1, F2, vbPrevMatched, vnMatches12, windowSize) --
 * Tracking::MonocularInitialization (Tracking.cc:2684-2688: the initial frame against the current one, window 100, nnratio 0.9, orientation
 * checked) -- END TO END on the device for `npairs` (initial frame row, current frame row, vbPrevMatched row) triples
 * (ORBmatcher.cc:799-943).  Two pools of rows as in orbm_search_for_triangulation_batch_async: pool 1 (initial frames) has nrows1 rows of
 * cap1 slots -- kps1 (mvKeysUn), desc1 [..][32], counts1 [nrows1] --, pool 2 (current frames) the same arrays with nrows2 / cap2 plus the grid
 * of orbm_grid_build_batch_async over the pool (grid_start [nrows2][3073], grid_idx [nrows2][cap2], indexed by row; min_x, min_y, inv_w,
 * inv_h as given there): the grid is how the search reaches a slot, so slots at or beyond a row's count are never read.  An extractor
 * result block is a valid pool; a caller with one pool passes it twice.  Pair p matches row row1[p] of pool 1 against row row2[p] of pool
 * 2; NULL = row p.  prev_in [npairs][cap1][2] is vbPrevMatched of pair p (x, y per F1 keypoint; after Tracking.cc:2635-2637 the initial
 * frame's own mvKeysUn[i].pt).  Semantics per pair are exactly those of orbm_search_for_initialization, line for line :799-943:
 *  - level-0 rule: only F1 keypoints with octave == 0 search (:825 skips level1 > 0), and they see only octave == 0 slots of F2:
 *    GetFeaturesInArea(prev.x, prev.y, window_size, 0, 0) checks the levels, walks the grid cells column-major and a cell's slots in
 *    insertion order, and keeps |dx| < window_size and |dy| < window_size, both strict.  (An octave below 0 searches every level, as the
 *    generic level rule of Frame.cc:828 says; no extractor produces one.)
 *  - the vMatchedDistance skip: a candidate whose slot is already claimed at a distance <= this one is passed over (:853), BEFORE best
 *    and second are updated, so a query may accept its second-nearest slot; best and second use strict <, the first candidate of least
 *    distance in visiting order wins; accepted when bestDist <= TH_LOW and bestDist < (float)bestDist2 * nnratio (float32 product,
 *    bestDist2 = INT_MAX without a second).  A claim of an owned slot is a steal: the former owner's vnMatches12 becomes -1 (:876-880).
 *  - the robbed-entry histogram rule: with check_orientation, rot = angle1 - angle2 (+360 if negative), bin = round(rot * (30 / 360.0f)),
 *    bin 30 -> 0, is counted WHEN THE CLAIM IS MADE and never taken back -- rotHist keeps a query that was robbed later (:902) -- so
 *    ComputeThreeMaxima sees bin sizes that cannot be recomputed from the finished row; culling a robbed entry does not count down a
 *    second time (:926).  A bin outside [0, 30) (a NaN angle; the reference asserts) is neither counted nor culled.
 * Outputs (device): matches12 [npairs][cap1] = vnMatches12 (idx2 or ORBM_NO_MATCH; slots at or beyond the row's count are ORBM_NO_MATCH),
 * nmatches [npairs] = the return value, prev_out [npairs][cap1][2] = vbPrevMatched after :938-940: entries below the row's count that
 * ended matched carry the matched F2 keypoint's position, the others carry prev_in's value; entries at or beyond the count are not
 * written.  In-place prev: prev_out == prev_in is allowed, as the reference updates vbPrevMatched in place -- replaying a captured graph
 * in place is then NOT idempotent (every replay searches around the last replay's matches, which is what the initialiser wants from frame
 * to frame); a caller who wants idempotent replays passes two buffers.  Partly overlapping buffers are not allowed.  A pair whose row1 or
 * row2 lies outside [0, nrows1) / [0, nrows2), or whose row is empty, gets count 0 and an all ORBM_NO_MATCH row.  The decisions around the
 * search stay with the caller (MonocularInitialization on the device).  All pointers are device pointers; enqueue-only:
 * the handle's work buffer (the candidate lists of the pairs in flight) is min(npairs, 128) * (cap2 + 262144) * 4 bytes of device memory
 * -- 1.1 MB per pair in flight at cap2 = 5 000, 68 MB for 64 such pairs, 151 MB at most (128 pairs at the cap) --, grow-only and kept for
 * the handle's life; it is allocated by the first eager call and reused, so after one eager call of the same or a smaller shape the
 * call can be captured (orbx_capture_begin) and allocates nothing.  There is no cap on
 * the candidates of a query: a window that holds every level-0 slot of the row works (the lists are produced and consumed in chunks of
 * queries).  ORBM_E_INVALID: a NULL required array (row1 / row2 may be NULL), npairs, nrows1, nrows2, cap1 or cap2 < 1, window_size < 0;
 * ORBM_E_CAPACITY: cap1 or cap2 > ORBM_INIT_MAX_CAP (16-bit owner indices; the claimed row over cap2 takes 4 B per slot of the 160 KB of
 * LDS), npairs > 65535.  Nothing is enqueued then. */
enum { ORBM_INIT_MAX_CAP = 32768 };
int orbm_search_for_initialization_batch_async(orbm_t*, int npairs,
                                               int nrows1, int cap1, const orbm_kp_t* kps1, const uint8_t* desc1, const int32_t* counts1,
                                               int nrows2, int cap2, const orbm_kp_t* kps2, const uint8_t* desc2, const int32_t* counts2,
                                               const int32_t* grid_start, const int32_t* grid_idx, float min_x, float min_y, float inv_w, float inv_h,
                                               const int32_t* row1, const int32_t* row2, const float* prev_in,
                                               int window_size, float nnratio, int check_orientation,
                                               int32_t* matches12, int32_t* nmatches, float* prev_out);

/* ---- RGB-D frames (the third sensor family: Frame's RGB-D constructor, Frame.cc:228-314).
 * orbm_stereo_from_rgbd / orbm_stereo_from_rgbd_batch_async: Frame::ComputeStereoFromRGBD (Frame.cc:1279-1309) with
 * Tracking::GrabImageRGBD's imDepth.convertTo(imDepth, CV_32F, mDepthMapFactor) (Tracking.cc:1353-1354) folded into the sample: the
 * caller passes the UNCONVERTED depth image and mDepthMapFactor; only the pixels under keypoints are read, and converting one pixel gives
 * the value converting the image gives.  Per keypoint i, line for line :1288-1308:
 *  - Pixel: row = (int)kps[i].y, col = (int)kps[i].x -- the float-to-int truncation that imDepth.at<float>(v, u) performs on its float
 *    arguments (towards zero, so a coordinate in (-1, 0) reads index 0).  kps is mvKeys, the raw keypoints; kps_un is mvKeysUn and may be
 *    the same array when there is no distortion.  A keypoint whose row or column lies outside the image, or whose coordinate is NaN,
 *    reads nothing and gets uright = depth = -1; the reference reads out of bounds there.
 *  - Conversion: the raw pixel is used as it is only when depth_type == ORBM_DEPTH_F32 and fabs(depth_factor - 1.0f) > 1e-5 is false
 *    (:1353 as written); in every other case d = (float)raw * depth_factor, one float32 multiply without contraction and without an
 *    offset -- what cv::Mat::convertTo yields for 16U -> 32F and 32F -> 32F with beta == 0.
 *  - Result: d > 0 gives depth[i] = d and uright[i] = kps_un[i].x - mbf / d (float32 IEEE division, then a float32 subtraction);
 *    otherwise both are -1.0f: 0, negatives and NaN.  +inf passes: uright = kps_un[i].x.
 * depth_img / the images: rows of stride_bytes bytes, w x h elements of uint16 (ORBM_DEPTH_U16) or float (ORBM_DEPTH_F32), aligned to the
 * element; stride_bytes is a multiple of the element size, as every cv::Mat step is.
 * Host form: host pointers, one frame, synchronous; uright / depth [n]; returns the number of keypoints with depth > 0.
 * Device form: enqueue-only, all pointers device pointers.  Frame f of the call is block frame first + f of kps, kps_un and counts -- an
 * extractor result block (orbx_result_device) and the block orbm_undistort_keypoints(ORBM_DEVICE) wrote from it, rows of cap slots.
 * depth_imgs is a DEVICE array of nframes device pointers: a captured graph follows a caller who rewrites the table (or the pixels)
 * between replays.  Outputs have one row per frame of the call: uright, depth [nframes][cap], with slots at or beyond the frame's count
 * written -1 as well, so a row is fully defined; nvalid [nframes] = keypoints with depth > 0.  The rows follow the convention of the
 * uright that orbm_stereo_batch_async writes: they go straight into orbm_search_by_projection_frame_batch_async (M4, with mbf) and
 * orbm_search_by_projection_points_batch_async (M3) when t_first == first.  nvalid is computed from the finished row (one workgroup per
 * frame; ballot, popcount, LDS reduction, one store): nothing accumulates across graph replays and nothing needs a memset.  No scratch:
 * capturable after one eager call (orbx_capture_begin), as the other batched forms.
 * ORBM_E_INVALID, with nothing enqueued: a NULL array; nframes, cap, w or h < 1; first < 0; stride_bytes < w * element size or not a
 * multiple of it; an unknown depth_type; a non-finite depth_factor. */
enum { ORBM_DEPTH_U16 = 0, ORBM_DEPTH_F32 = 1 };
int orbm_stereo_from_rgbd(orbm_t*, int n, const orbm_kp_t* kps, const orbm_kp_t* kps_un,
                          const void* depth_img, int depth_type, int w, int h, int stride_bytes,
                          float depth_factor, float mbf, float* uright, float* depth);
int orbm_stereo_from_rgbd_batch_async(orbm_t*, int nframes, int first, int cap,
                                      const orbm_kp_t* kps, const orbm_kp_t* kps_un, const int32_t* counts,
                                      const void* const* depth_imgs, int depth_type, int w, int h, int stride_bytes,
                                      float depth_factor, float mbf,
                                      float* uright, float* depth, int32_t* nvalid);
/* orbm_unproject_stereo / orbm_unproject_stereo_batch_async: Frame::UnprojectStereo (Frame.cc:1312-1326) for every keypoint of a frame
 * -- what StereoInitialization, UpdateLastFrame and CreateNewKeyFrame call per depth point in RGB-D and stereo tracking.  k / k_host =
 * (fx, fy, cx, cy) on the host; twc is the row-major 3x4 [Rwc | Ow] (mRwc, mOw).  Per slot with z = depth > 0 (:1314-1322): invfx =
 * 1.0f / fx computed once; x = (u - cx) * z * invfx evaluated left to right in float without contraction, y likewise, (u, v) =
 * kps_un.pt; x3Dw[r] = (float)(double sum over k of Rwc[r][k] * x3Dc[k]) + Ow[r], the cv::Mat product rule of facade/cvcompat.h as
 * orbm_project_last_frame_batch_async states it (not the Matx rule of orbm_is_in_frustum); has_depth = 1.  Any other slot (0, negative,
 * NaN; the reference returns an empty Mat) gets has_depth = 0 and x3dw = (0, 0, 0).
 * Host form: host pointers, one frame, synchronous; x3dw [n][3], has_depth [n]; returns the number of points.
 * Device form: enqueue-only, device pointers except k_host.  Row r of the call is block frame first + r of kps_un and counts (rows of
 * cap); depth [nrows][cap] has one row per row of the call, as orbm_stereo_from_rgbd_batch_async and orbm_stereo_batch_async write it;
 * twc [nrows][12] is device data, so a replay follows new poses.  Outputs x3dw [nrows][cap][3], has_depth [nrows][cap]; slots at or
 * beyond the count get 0 and (0, 0, 0) too.  With q_stride == cap they are valid x3dw / has_mp inputs of
 * orbm_project_last_frame_batch_async.  Which depth points become temporal MapPoints stays with the caller (UpdateLastFrame takes the
 * 100 closest and those under mThDepth): the caller ANDs its own selection into has_depth.  No scratch: capturable after one eager
 * call (orbx_capture_begin).  ORBM_E_INVALID: a NULL array, nrows or cap < 1, first < 0; ORBM_E_CAPACITY: nrows > 65535.
 * That selection is also available on the device: orbm_select_depth_points_batch_async and orbm_adopt_new_points_batch_async below. */
int orbm_unproject_stereo(orbm_t*, int n, const orbm_kp_t* kps_un, const float* depth, const float* twc12,
                          const float* k, float* x3dw, uint8_t* has_depth);
int orbm_unproject_stereo_batch_async(orbm_t*, int nrows, int first, int cap, const orbm_kp_t* kps_un, const int32_t* counts,
                                      const float* depth, const float* twc, const float* k_host,
                                      float* x3dw, uint8_t* has_depth);
/* orbm_select_depth_points / orbm_select_depth_points_batch_async: which depth points of a stereo / RGB-D frame become MapPoints -- the
 * sorted walk that Tracking::UpdateLastFrame (Tracking.cc:3094-3163, temporal points before TrackWithMotionModel) and
 * Tracking::CreateNewKeyFrame (Tracking.cc:3694-3783, the new points of every stereo / RGB-D KeyFrame) both run -- and the close counts
 * of Tracking::NeedNewKeyFrame (Tracking.cc:3524-3546) over the same mvDepth row and threshold.  For one frame with n slots:
 *  - D = { i < n : mvDepth[i] > 0 }: NaN, 0 and negatives are out; +inf is in, as orbm_stereo_from_rgbd passes it; a positive denormal
 *    is in (the test runs on the bit pattern, nothing is flushed).
 *  - D is sorted as std::pair<float,int>: ascending depth, equal depths in ascending slot order (ties by slot).  Slots are unique, so
 *    the order is total and the result deterministic.
 *  - The walk visits the sorted points in order and stops after visiting the first position j with depth_j > th_depth && j + 1 >
 *    max_points (nPoints is incremented in both branches, so it is j + 1).  With c = the number of points of D with !(depth >
 *    th_depth): nvisit = min(|D|, max(c, max_points) + 1) -- one extra point beyond the bound is visited as well: 150 far points and
 *    max_points = 100 give 101 visited slots, not 100.  A NaN th_depth never stops the walk (nvisit = |D|).  max_points is the
 *    reference's 100 (maxPoint).
 *  - A visited slot creates a new point when it holds no MapPoint or one with Observations() < 1: create_new = visited && !keeps_mp,
 *    where keeps_mp is the caller's `pMP && pMP->Observations() >= 1` (NULL = no slot holds one).  Other visited slots only advance
 *    the walk.
 *  - Close counts: slots with depth > 0 && depth < th_depth, split by tracked = `mvpMapPoints[i] && !mvbOutlier[i]` (NULL = none) into
 *    nclose_tracked and nclose_untracked.  Mind the strict < here against the > of the walk: a depth equal to th_depth is in neither
 *    close count, yet it does not stop the walk.  With a NaN th_depth both counts are 0.
 * Outputs: order[j] = the slot visited at position j < nvisit, -1 for the rest of the row; create_new per slot (0 where not visited);
 * nvisit, ncreate = the number of create_new slots; nclose_tracked / nclose_untracked may be NULL.  The caller creates its MapPoints
 * in `order`, which is the order the reference creates them in (and so the order of their ids).
 * Host form: host pointers, one frame of n slots, synchronous; order [n], create_new [n]; ncreate, nclose_tracked and nclose_untracked
 * point to one int each and may be NULL; returns nvisit.
 * Device form: enqueue-only, all pointers device pointers.  Row r of the call uses counts[first + r] (an extractor result block's
 * counts; n = min(max(count, 0), cap)) and row r of depth [nrows][cap] -- one row per row of the call, as
 * orbm_unproject_stereo_batch_async reads it and orbm_stereo_from_rgbd_batch_async / orbm_stereo_batch_async write it -- of keeps_mp
 * and tracked [nrows][cap], and writes row r of order, create_new [nrows][cap] and entry r of nvisit, ncreate, nclose_tracked,
 * nclose_untracked [nrows].  Slots at or beyond the count are never visited, whatever their depth / keeps_mp hold; their create_new is
 * written 0 and their order -1, so the rows are fully defined.  One workgroup per row sorts 64-bit keys (depth bits << 32 | slot) in
 * LDS, sized from cap padded to a power of two; every count is written from the finished row with plain stores:
 * nothing accumulates across graph replays and nothing needs a memset.  No scratch: capturable after one eager call
 * (orbx_capture_begin).
 * Limit: cap (host form: n) <= ORBM_DEPTH_SELECT_MAX_CAP = 16384 -- 128 KiB of keys out of the 160 KiB of LDS; stereo and RGB-D
 * extractors never use the 5 x nFeatures initialiser.
 * ORBM_E_INVALID, with nothing enqueued: a NULL required array; nrows or cap < 1 (host form: n < 0); first < 0; max_points < 0.
 * ORBM_E_CAPACITY, with nothing enqueued: cap above the limit or nrows > 65535.
 *
 * orbm_adopt_new_points_batch_async: `new MapPoint(x3D, pMap, &mLastFrame, i)` + `mLastFrame.mvpMapPoints[i] = pNewMP`
 * (Tracking.cc:3139-3143) as far as M4 reads it, thread per slot, pinhole (Nleft == -1).  Row r of the call is block frame first + r of
 * counts and desc (the block's descriptor rows [..][cap][32]); create_new [nrows][cap] as the select call wrote it; x3d_new
 * [nrows][cap][3] the rows orbm_unproject_stereo_batch_async wrote; outlier [nrows][cap] = mvbOutlier (NULL = none).  In/out rows, one
 * per row of the call: x3dw [nrows][cap][3], has_mp, mp_obs [nrows][cap], qdesc [nrows][cap][32].  Where create_new is set and the slot
 * lies below the count: x3dw = x3d_new; has_mp = !outlier (M4 tests pMP && !mvbOutlier[i], ORBmatcher.cc:2505-2509); mp_obs = 0 (the
 * constructor sets nObs(0), MapPoint.cc:92); qdesc = the frame's own descriptor row of that slot (MapPoint.cc:127).  Every other slot is
 * untouched.  With q_stride == cap the four rows are then inputs of orbm_project_last_frame_batch_async and
 * orbm_search_by_projection_frame_batch_async as they stand.  desc and qdesc are read / written as 32-bit words: 4-byte aligned.
 * For CreateNewKeyFrame the map surgery (AddObservation, AddMapPoint, the Atlas), the UnprojectStereoFishEye branch and the
 * mvLeftToRightMatch partner slot stay with the caller.  No scratch: capturable.  ORBM_E_INVALID: a NULL array other than outlier, nrows
 * or cap < 1, first < 0; ORBM_E_CAPACITY: nrows > 65535. */
enum { ORBM_DEPTH_SELECT_MAX_CAP = 16384 };
int orbm_select_depth_points(orbm_t*, int n, const float* depth, const uint8_t* keeps_mp, const uint8_t* tracked,
                             float th_depth, int max_points, int32_t* order, uint8_t* create_new,
                             int32_t* ncreate, int32_t* nclose_tracked, int32_t* nclose_untracked);
int orbm_select_depth_points_batch_async(orbm_t*, int nrows, int first, int cap, const int32_t* counts, const float* depth,
                                         const uint8_t* keeps_mp, const uint8_t* tracked, float th_depth, int max_points,
                                         int32_t* order, uint8_t* create_new, int32_t* nvisit, int32_t* ncreate,
                                         int32_t* nclose_tracked, int32_t* nclose_untracked);
int orbm_adopt_new_points_batch_async(orbm_t*, int nrows, int first, int cap, const int32_t* counts, const uint8_t* create_new,
                                      const float* x3d_new, const uint8_t* desc, const uint8_t* outlier,
                                      float* x3dw, uint8_t* has_mp, uint8_t* mp_obs, uint8_t* qdesc);

/* ---- MapPoint refresh: the producer of the qdesc / normal / min_dist / max_dist rows that the batched searches read (M3, M4, M5, M6,
 * M13, orbm_is_in_frustum), for a batch of MapPoints over a resident pool of KeyFrame rows.
 * Shared inputs.  KeyFrame pool, the orbm_fuse_batch_async convention: nkf_rows rows of cap slots, desc_kf [nkf_rows][cap][32], kps_kf
 * [nkf_rows][cap], counts_kf [nkf_rows]; a two-camera KeyFrame is ONE stacked row (left slots, then right, as mDescriptors after vconcat),
 * so the reference's rightIndex is already a slot of the row.  ow_l [nkf_rows][3] = GetCameraCenter, ow_r [nkf_rows][3] =
 * GetRightCameraCenter per row; ow_r may be NULL when no entry names the right camera (an entry that does so anyway is then skipped).
 * Observations, a CSR over the MapPoints of the call: obs_off [nmp + 1] absolute offsets into obs_row / obs_slot / obs_flags [nobs]
 * (obs_off[0] may be non-zero); per entry the pool row, the slot in that row and flags: bit 0 = a right-camera observation, bit 1 = the
 * KeyFrame isBad().  The caller lays out a MapPoint's entries in the order its mObservations map is walked, the left entry before the
 * right entry of the same KeyFrame (MapPoint.cc:481-486, :610-621); that order is pointer order in the reference, so the contract is "in
 * the order given".  valid [nmp] is the !mbBad test (NULL = all valid): for a MapPoint that is not valid none of its rows is read.
 * Skip rules (defined here, not by the reference): an entry is skipped by both functions when obs_row lies outside [0, nkf_rows) or
 * obs_slot outside [0, min(counts_kf[row], cap)); a non-increasing obs_off pair, a pair that leaves [0, nobs] and a list of more than
 * ORBM_MP_MAX_OBS entries are an empty list.  Nothing reads out of bounds on device data.
 * Alignment: desc_kf must be 16-byte aligned (descriptor rows are read as two 128-bit words) and mp_desc 4-byte aligned (rows are
 * written as eight 32-bit words); every other array is aligned to its element.  A sub-buffer that starts at a whole descriptor row of
 * an allocation aligned to 32 bytes meets both.
 *
 * orbm_distinctive_descriptors / orbm_distinctive_descriptors_batch_async: MapPoint::ComputeDistinctiveDescriptors
 * (MapPoint.cc:450-538).  Entries with bit 1 set are skipped as well (:477).  Over the N remaining descriptors every pairwise
 * DescriptorDistance is taken; per row i the N distances, the 0 to itself included, are ordered and element (int)(0.5 * (N - 1)) is the
 * row's median (:518-521): the lower median for even N.  Tie rule: the FIRST row of least median wins (strict <, :524).  A distance of
 * 256 is a legal value (a descriptor and its complement) and is kept in 16 bits: it never wraps to 0.  Outputs: mp_desc [nmp][32] = the
 * winning descriptor; best_obs [nmp] = the winner's position in the MapPoint's own entry list, skipped entries counted, or -1;
 * best_median [nmp] (optional, NULL = not written) = 0..256, or -1.  With N == 0, or a MapPoint that is not valid, mp_desc keeps the
 * caller's bytes (the reference returns without touching mDescriptor) and best_obs / best_median are -1.  There is no cap on N up to
 * ORBM_MP_MAX_OBS = 65535: nothing is truncated and nothing falls back to the host (one wave per MapPoint; lists beyond 64 entries are
 * walked in chunks of 64 rows by the four waves of the MapPoint's workgroup).  mp_desc is a valid qdesc of the batched searches when nmp matches their npairs * q_stride layout.
 *
 * orbm_update_normal_and_depth / orbm_update_normal_and_depth_batch_async: MapPoint::UpdateNormalAndDepth (MapPoint.cc:578-652).  Bad
 * KeyFrames are NOT skipped here (the reference does not test them).  Numerics are the facade's lines against facade/cvcompat.h: per
 * entry, in list order, d = pw - Ow in float (Ow from ow_l, or ow_r with bit 0), s = (float)(1.0 / sqrt(double sum of d^2)), normal =
 * normal + d * s as a float multiply then a float add without contraction, n++; the sum is sequential per MapPoint, float addition order
 * is part of the result.  Then dist = (float)sqrt(double sum of (pw - ow_l[ref_row])^2), level = kps_kf[ref_row][ref_slot].octave (the
 * caller picks ref_slot by the rules of :627-638), max_dist = dist * scale[level], min_dist = max_dist / scale[nlevels - 1], normal_out =
 * normal * (float)(1.0 / n).  pw [nmp][3], ref_row / ref_slot [nmp]; scale_factors(_host) [nlevels] on the host.  Outputs normal
 * [nmp][3], min_dist, max_dist, updated [nmp].  updated = 0, with that MapPoint's three rows left untouched, when the MapPoint is not
 * valid, n == 0, ref_row or ref_slot is out of range, or the octave lies outside [0, nlevels).  A point exactly at a camera centre gives
 * inf or NaN by IEEE; the bits of a NaN are not pinned.  The rows go straight into orbm_is_in_frustum(ORBM_DEVICE) and the min_dist /
 * max_dist / normal inputs of the batched projections.
 *
 * Host forms: host pointers, synchronous; mp_desc / normal / min_dist / max_dist are in/out (rows that are not written keep the caller's
 * values); return the number of MapPoints that got a descriptor / were updated.  Device forms: enqueue-only, all pointers device pointers
 * except scale_factors_host; no work buffer, every output is recomputed per launch and nothing accumulates across graph replays, so the
 * calls can be captured (orbx_capture_begin) at once.  ORBM_E_INVALID, with nothing enqueued: a NULL required array (valid, ow_r and
 * best_median may be NULL); nmp, nkf_rows, cap or nlevels < 1; nobs < 0.  ORBM_E_CAPACITY: nlevels > 12, nmp > ORBM_MP_MAX_BATCH,
 * nkf_rows * cap > 2^31 - 1. */
enum { ORBM_MP_MAX_OBS = 65535, ORBM_MP_MAX_BATCH = 1 << 20 };
int orbm_distinctive_descriptors(orbm_t*, int nmp, int nkf_rows, int cap, const uint8_t* desc_kf, const int32_t* counts_kf,
                                 int nobs, const int32_t* obs_off, const int32_t* obs_row, const int32_t* obs_slot,
                                 const uint8_t* obs_flags, const uint8_t* valid,
                                 uint8_t* mp_desc, int32_t* best_obs, int32_t* best_median);
int orbm_distinctive_descriptors_batch_async(orbm_t*, int nmp, int nkf_rows, int cap, const uint8_t* desc_kf, const int32_t* counts_kf,
                                             int nobs, const int32_t* obs_off, const int32_t* obs_row, const int32_t* obs_slot,
                                             const uint8_t* obs_flags, const uint8_t* valid,
                                             uint8_t* mp_desc, int32_t* best_obs, int32_t* best_median);
int orbm_update_normal_and_depth(orbm_t*, int nmp, int nkf_rows, int cap, const orbm_kp_t* kps_kf, const int32_t* counts_kf,
                                 const float* ow_l, const float* ow_r,
                                 int nobs, const int32_t* obs_off, const int32_t* obs_row, const int32_t* obs_slot,
                                 const uint8_t* obs_flags, const uint8_t* valid,
                                 const float* pw, const int32_t* ref_row, const int32_t* ref_slot, const float* scale_factors, int nlevels,
                                 float* normal, float* min_dist, float* max_dist, uint8_t* updated);
int orbm_update_normal_and_depth_batch_async(orbm_t*, int nmp, int nkf_rows, int cap, const orbm_kp_t* kps_kf, const int32_t* counts_kf,
                                             const float* ow_l, const float* ow_r,
                                             int nobs, const int32_t* obs_off, const int32_t* obs_row, const int32_t* obs_slot,
                                             const uint8_t* obs_flags, const uint8_t* valid,
                                             const float* pw, const int32_t* ref_row, const int32_t* ref_slot, const float* scale_factors_host, int nlevels,
                                             float* normal, float* min_dist, float* max_dist, uint8_t* updated);

/* ---- KeyFrameDatabase queries: which KeyFrames go into the batched searches.  KeyFrameDatabase::DetectRelocalizationCandidates
 * (KeyFrameDatabase.cc:869-981, caller Tracking.cc:4163) and DetectNBestCandidates (:660-866, caller LoopClosing.cc:592) up to and
 * including the scores; the covisibility accumulation over the three result rows is facade/KeyFrameDatabase.h.
 *
 * orbm_bow_vector_batch_async: mBowVec rows on the device.  word_id / weight [nrows][cap] are the rows orbm_bow_transform_batch_async
 * writes; counts [nrows], min(counts[r], cap) features per row (a negative count is 0).  Semantics: TemplatedVocabulary::transform for the
 * header `0 0` (TemplatedVocabulary.h:1145-1161, :1193) with BowVector::addWeight and normalize (BowVector.cpp:34-46, :62-84): a feature
 * with !(w > 0) is left out (zero, negative, NaN; :1157) -- so is one with a negative word id, which no transform writes --; the weights
 * of one word are added in feature order; norm is the double sum of fabs in ascending word id; every value is divided by norm only if
 * norm > 0.0.  Both sums are serial chains (double addition is not associative): one lane per word, one chain per row, nothing is
 * reassociated, so the rows equal the host's orbm_bow_vectors bit for bit.  Outputs bow_word [nrows][cap] ascending and unique, bow_val
 * [nrows][cap], nbow [nrows]; slots at or beyond nbow[r] keep the caller's bytes.  bow_val must not overlap weight.  Enqueue-only; no
 * work buffer, every value is recomputed per launch and nothing accumulates across graph replays; capturable (orbx_capture_begin) after
 * one eager call on the handle (the first call raises the kernel's LDS limit).  ORBM_E_INVALID: a NULL array, nrows or cap < 1.
 * ORBM_E_CAPACITY: cap > ORBM_BOWVEC_MAX_CAP = 16384 (a row's 64-bit keys word << 32 | slot are sorted in LDS), nrows > 65535.  All
 * checks run before anything is enqueued.
 *
 * orbm_kfdb_query (host pointers, synchronous) / orbm_kfdb_query_batch_async (device pointers, enqueue-only): one parameter list.
 * The database is a pool of BowVector rows in the layout above: db_word / db_val [ndb_rows][db_cap], db_n [ndb_rows]; the row index is
 * the order of the KeyFrameDatabase::add calls (:40-47).  db_active [ndb_rows] is 0 for a KeyFrame removed by erase / clearMap (:50-70,
 * :79-103); NULL = all active.  Queries are rows q_row[q], q < nq, of a second pool q_word / q_val [nq_rows][q_cap], q_n [nq_rows], which
 * may be the same arrays.  exclude [nq][ndb_rows] is spConnectedKF.count(pKFi) of DetectNBestCandidates (:692); NULL = none, the
 * relocalization form.  Row lengths are clamped with min(n, cap) (negative = 0); rows must ascend as orbm_bow_vector_batch_async writes
 * them.  Per query q and row r, with S = the words present in both vectors:
 *   common [nq][ndb_rows]      |S| (mnRelocWords :890 / mnPlaceRecognitionWords :701); 0 for inactive or excluded rows
 *   first_word [nq][ndb_rows]  the smallest word of S, -1 when common is 0
 *   max_common [nq]            the maximum of common over the rows (:898-903, :717-722)
 *   min_common [nq]            (int)((float)max_common * 0.8f): a float multiply with no contraction, then truncation (:905, :724)
 *   nsharing [nq]              rows with common > 0 = lKFsSharingWords.size()
 *   scored [nq][ndb_rows]      common > min_common, strict (:916, :739);  nscored [nq] = rows with scored set
 *   score [nq][ndb_rows]       where scored: (float)(-s / 2.0), s = L1Scoring::score's double sum of fabs(vi - wi) - fabs(vi) - fabs(wi)
 *                              over S in ascending word order (ScoringObject.cpp:23-68), vi from the query and wi from the row;
 *                              0.0f where scored is 0
 * With nsharing == 0 every output of that query is 0 / -1 (:894, :712).
 * List order.  The reference's lKFsSharingWords is exactly the rows with common > 0 sorted by (first_word, r): the inverted-file walk
 * visits the query's words in ascending order and each word's list in add order (:877-891, :675-709), and a KeyFrame enters the list at
 * the first word it shares, its first_word; KeyFrames that enter at one word do so in that word's list order, which is add order = row
 * order.  So a stable sort of the sharing rows by first_word rebuilds the list, and with it the order of lScoreAndMatch.
 * The intersection is parallel (a wave per (query, row), binary search in the query's words); the sum is one serial chain per scored
 * row in word order.  max_common, nsharing and nscored are reduced across rows with integer atomics and are zeroed by memsets inside
 * the enqueued work, so a replayed graph starts clean; no scratch.  Capturable at once.  ORBM_E_INVALID: a NULL required array
 * (db_active and exclude may be NULL); nq, nq_rows, q_cap, ndb_rows or db_cap < 1; in the host form a q_row entry outside [0, nq_rows).
 * In the device form such a query writes the empty result (all 0 / -1).  ORBM_E_CAPACITY: q_cap or db_cap > 65535, ndb_rows >
 * ORBM_KFDB_MAX_ROWS, nq > ORBM_KFDB_MAX_QUERIES.  All checks run before anything is enqueued and leave the outputs untouched.  Nothing
 * reads out of bounds.  No CPU fallback: ORBM_E_HIP without a device.  Both return ORBM_OK. */
enum { ORBM_BOWVEC_MAX_CAP = 16384 };
enum { ORBM_KFDB_MAX_ROWS = 1 << 20, ORBM_KFDB_MAX_QUERIES = 65535 };
int orbm_bow_vector_batch_async(orbm_t*, const int32_t* word_id, const double* weight, const int32_t* counts, int nrows, int cap,
                                int32_t* bow_word, double* bow_val, int32_t* nbow);
int orbm_kfdb_query(orbm_t*, int nq, const int32_t* q_row,
                    int nq_rows, int q_cap, const int32_t* q_word, const double* q_val, const int32_t* q_n,
                    int ndb_rows, int db_cap, const int32_t* db_word, const double* db_val, const int32_t* db_n,
                    const uint8_t* db_active, const uint8_t* exclude,
                    int32_t* common, int32_t* first_word, float* score, uint8_t* scored,
                    int32_t* max_common, int32_t* min_common, int32_t* nsharing, int32_t* nscored);
int orbm_kfdb_query_batch_async(orbm_t*, int nq, const int32_t* q_row,
                                int nq_rows, int q_cap, const int32_t* q_word, const double* q_val, const int32_t* q_n,
                                int ndb_rows, int db_cap, const int32_t* db_word, const double* db_val, const int32_t* db_n,
                                const uint8_t* db_active, const uint8_t* exclude,
                                int32_t* common, int32_t* first_word, float* score, uint8_t* scored,
                                int32_t* max_common, int32_t* min_common, int32_t* nsharing, int32_t* nscored);

/* ---- KeyFrameCulling: the redundancy counts of LocalMapping::KeyFrameCulling (LocalMapping.cc:1218-1400) for every covisible KeyFrame
 * of the new one in ONE call, over the arrays the MapPoint refresh already keeps resident.
 * orbm_keyframe_culling (host pointers, synchronous) / orbm_keyframe_culling_batch_async (device pointers, enqueue-only): one parameter
 * list.
 * Inputs.  The KeyFrame pool kps_kf [nkf_rows][cap], counts_kf [nkf_rows] and the observation CSR obs_off [nmp + 1] / obs_row / obs_slot
 * / obs_flags [nobs] follow the MapPoint refresh convention exactly: a two-camera KeyFrame is one stacked row, an entry is skipped when
 * obs_row lies outside [0, nkf_rows) or obs_slot outside [0, min(counts_kf[row], cap)), a non-increasing obs_off pair, a pair that leaves
 * [0, nobs] and a list of more than ORBM_MP_MAX_OBS entries are an empty list.  cand_row [ncand] = the pool rows of the candidates in the
 * order of GetVectorCovisibleKeyFrames(); the caller leaves out the KeyFrames the reference skips (mnId == GetInitKFid() || isBad(),
 * :1272).  kf_mp [ncand][cap] = per candidate slot the index of GetMapPointMatches()[i] in the call's MapPoint list; an index outside
 * [0, nmp) means NULL.  depth [ncand][cap] = mvDepth; NULL means mbMonocular, no gate.  mp_valid [nmp] = !isBad(); NULL = all valid.
 * mp_nobs [nmp] = Observations().  erased [nkf_rows] marks erased KeyFrames; NULL = none.  th_obs is 3; redundant_th is 0.9f or 0.5f
 * (:1238-1245).
 * Entry flags.  Bit 2 of obs_flags: the entry weighs 2 in nObs (!pKF->mpCamera2 && mvuRight[leftIndex] >= 0, MapPoint.cc:212, :232);
 * otherwise it weighs 1.  The two refresh calls ignore bit 2.  Bit 1 (the KeyFrame isBad()) is ignored here: the reference does not test
 * it.  Bit 0 = a right-camera observation, as before.
 * Semantics.  Candidate k has r = cand_row[k] and walks the slots i < min(counts_kf[r], cap); a candidate with r out of range or
 * erased[r] set gives zeros.  In this order:
 *   1. j = kf_mp[k][i]; j NULL or mp_valid[j] == 0: the slot is not counted.
 *   2. Over the live entries of MapPoint j (after the skip rules) E is the set of entries whose row is erased; nobs_eff = mp_nobs[j] -
 *      the sum of the weights of E.  If E is not empty and nobs_eff <= 2 the MapPoint is bad by erasure and the slot is not counted
 *      (MapPoint::EraseObservation, MapPoint.cc:220-257; MapPoint::SetBadFlag, :280-305).  nObs only falls, so testing the final value
 *      equals the reference's test after each erase.
 *   3. depth != NULL and (depth[k][i] > th_depth || depth[k][i] < 0), the reference's expression as written (:1295): not counted.  A
 *      NaN depth is counted, -0.0 is counted, depth == th_depth is counted.
 *   4. n_mps[k]++.
 *   5. If nobs_eff > th_obs: L = kps_kf[r][i].octave, and the observing KeyFrames are counted.  An entry takes part if its row is not
 *      erased and is not r; it passes if its keypoint's octave <= L + 1.  A right entry (bit 0) directly preceded in the list by a left
 *      entry of the same row, both of them live, forms one KeyFrame with it, which counts once if either entry passes (the scaleLeveli
 *      minimum of :1316-1328).  Any other arrangement counts per entry: this is defined here, not by the reference.  If the count is >
 *      th_obs, n_redundant[k]++.  The reference's break at :1335 does not change the answer.
 *   6. cull[k] = (float)n_redundant > redundant_th * (float)n_mps: one float multiply and one compare, with no contraction (:1349).
 *      With 0.9f, 9 of 10 is not culled and 10 of 11 is.  first_cull (optional, NULL = not written) = the least k with cull[k] set, or -1.
 *   7. slot_state [ncand][cap] (optional, NULL = not written): 0 = not counted, 1 = counted, 2 = redundant.  Every slot below cap is
 *      written; 0 at and beyond the row's count.
 * Deviation.  For a two-camera candidate the reference reads mvKeysRight[i].octave with the stacked index i (:1303-1305): past the end
 * or the wrong feature.  The library reads slot i of the stacked row.
 * The sequential rule.  A KeyFrame that is voted out is erased at once (KeyFrame::SetBadFlag, KeyFrame.cc:746-887), so a later
 * candidate is counted on a changed map.  The results are exact for candidates 0 .. first_cull.  The caller then decides what to do
 * with candidate first_cull -- in inertial mode the mPrevKF / mNextKF / time tests (:1352-1387) stay with the caller --; if the KeyFrame
 * was really erased (isBad() afterwards; mbNotErase leaves it alive) the caller sets erased[row] = 1 and calls again for the remaining
 * candidates.  No CSR, pool or kf_mp row is rebuilt.  Only while erased is all zero or NULL does a single call equal the reference for
 * every candidate.  The rule assumes the map invariant that an observation entry of KeyFrame X exists exactly where X's mvpMapPoints
 * holds that MapPoint.
 * Outputs n_mps, n_redundant [ncand], cull [ncand], slot_state, first_cull [1].  The host form returns the number of candidates with
 * cull set; the device form returns ORBM_OK.  The device form uses no scratch that survives a call: the counts are summed with integer
 * atomics into n_mps / n_redundant, which memsets inside the enqueued work zero first, every output is recomputed per launch and nothing
 * accumulates across graph replays; it is capturable (orbx_capture_begin) from the first call, and a replay follows rewritten erased,
 * kf_mp, mp_valid, mp_nobs and cand_row rows.  With erased == NULL a list is left as soon as its count has passed th_obs; with an erased
 * row every list is walked to its end; the outputs are the same.  Nothing reads out of bounds whatever the indices hold.
 * ORBM_E_INVALID, with nothing enqueued: a NULL required array (depth, mp_valid, erased, slot_state and first_cull may be NULL); ncand,
 * nkf_rows, cap or nmp < 1; nobs < 0; th_obs < 0.  ORBM_E_CAPACITY: ncand > ORBM_KFCULL_MAX_CAND, cap > ORBM_KFCULL_MAX_CAP, nmp >
 * ORBM_MP_MAX_BATCH, nkf_rows * cap > 2^31 - 1.  No CPU fallback: ORBM_E_HIP without a device. */
enum { ORBM_KFCULL_MAX_CAND = 65535, ORBM_KFCULL_MAX_CAP = 65535 };
int orbm_keyframe_culling(orbm_t*, int ncand, const int32_t* cand_row, int nkf_rows, int cap,
                          const orbm_kp_t* kps_kf, const int32_t* counts_kf, const int32_t* kf_mp, const float* depth, float th_depth,
                          int nmp, int nobs, const int32_t* obs_off, const int32_t* obs_row, const int32_t* obs_slot, const uint8_t* obs_flags,
                          const uint8_t* mp_valid, const int32_t* mp_nobs, const uint8_t* erased, int th_obs, float redundant_th,
                          int32_t* n_mps, int32_t* n_redundant, uint8_t* cull, uint8_t* slot_state, int32_t* first_cull);
int orbm_keyframe_culling_batch_async(orbm_t*, int ncand, const int32_t* cand_row, int nkf_rows, int cap,
                                      const orbm_kp_t* kps_kf, const int32_t* counts_kf, const int32_t* kf_mp, const float* depth, float th_depth,
                                      int nmp, int nobs, const int32_t* obs_off, const int32_t* obs_row, const int32_t* obs_slot, const uint8_t* obs_flags,
                                      const uint8_t* mp_valid, const int32_t* mp_nobs, const uint8_t* erased, int th_obs, float redundant_th,
                                      int32_t* n_mps, int32_t* n_redundant, uint8_t* cull, uint8_t* slot_state, int32_t* first_cull);

/* ---- Covisibility votes and the local map: KeyFrame::UpdateConnections step 1 (KeyFrame.cc:474-512), the keyframeCounter of
 * Tracking::UpdateLocalKeyFrames (Tracking.cc:3964-4013), Tracking::UpdateLocalPoints (Tracking.cc:3917-3948) and the gather of the
 * query rows SearchLocalPoints reads, over the arrays the MapPoint refresh and KeyFrameCulling already keep resident.  Everything is
 * integer: results are exact.
 *
 * orbm_covisibility_votes (host pointers, synchronous) / orbm_covisibility_votes_batch_async (device pointers, enqueue-only): one
 * parameter list.
 * Inputs.  counts_kf [nkf_rows] and the observation CSR obs_off [nmp + 1] / obs_row / obs_slot / obs_flags [nobs] follow the MapPoint
 * refresh convention exactly: an entry is skipped when obs_row lies outside [0, nkf_rows) or obs_slot outside [0, min(counts_kf[row],
 * cap)), a non-increasing obs_off pair, a pair that leaves [0, nobs] and a list of more than ORBM_MP_MAX_OBS entries are an empty list.
 * The pool (nkf_rows, cap, counts_kf) is used only for the slot skip rule.  q_mp [nq][q_stride] = per query the MapPoint index of each
 * slot, q_n [nq] its slot count: min(q_n, q_stride) slots are read, a negative count reads as 0, an index outside [0, nmp) means NULL.
 * A query is a Frame's mvpMapPoints (UpdateLocalKeyFrames) or a KeyFrame's GetMapPointMatches() (UpdateConnections).  self_row [nq] =
 * the query KeyFrame's own pool row, whose entries do not vote (mnId == mnId, KeyFrame.cc:503); -1, or a NULL array, means no self
 * row, as for a Frame.  kf_skip [nkf_rows]: non-zero = entries of this row do not vote (the caller folds GetMap() != mpMap in here);
 * NULL = none.  mp_valid [nmp] = !isBad(); NULL = all valid.  th is 15 for UpdateConnections and is used only for n_over.
 * Entry flags.  Bit 0 of obs_flags = a right-camera entry.  Bit 1 = the KeyFrame isBad(): with skip_bad non-zero such an entry does
 * not vote (UpdateConnections passes 1); UpdateLocalKeyFrames passes 0, the reference counts a bad KeyFrame and drops it afterwards
 * (:4033).  Bit 2 is ignored here.
 * Semantics.  Each slot of a query votes, in any order, through its MapPoint, which must be non-NULL and valid.  Every live,
 * non-skipped entry of that MapPoint adds one vote to its row.  The reference's mObservations holds one entry per KeyFrame, so a right
 * entry directly preceded in the list by a live, non-skipped left entry of the same row adds nothing: the KeyFrame voted at the left
 * entry (the pair rule of KeyFrameCulling).  Any other arrangement votes per entry: this is defined here, not by the reference.  A
 * MapPoint that sits in two slots of a query votes twice, as the reference's loop over slots does.
 * Outputs.  votes [nq][nkf_rows] = the dense votes per query; n_voted [nq] = the number of rows with votes > 0; max_votes [nq] = the
 * maximum vote; n_over [nq] = the number of voted rows with votes >= th; list_row / list_votes [nq][list_cap] = the rows with votes > 0 in
 * ascending row order and their counts: the first min(n_voted, list_cap) entries are written and the rest of the row keeps the
 * caller's bytes; list_cap may be 0 with both pointers NULL.  The reference's tie rules stay with the caller (facade/Covisibility.h):
 * pKFmax is the first maximum in pointer order with strict >, sort(vPairs) runs on (weight, pointer) pairs; the library reports only
 * counts.  Both forms return ORBM_OK.
 * The device form uses no scratch: votes and the three count rows are zeroed by memsets inside the enqueued work, the votes are summed
 * with integer atomics (per workgroup in LDS first), every output is recomputed per launch and nothing accumulates across graph
 * replays; it is capturable (orbx_capture_begin) from the first call, and a replay follows rewritten q_mp, q_n, self_row and kf_skip
 * rows.  Nothing reads out of bounds whatever the indices hold.
 * ORBM_E_INVALID, with nothing enqueued: a NULL required array (self_row, kf_skip and mp_valid may be NULL; list_row / list_votes only
 * with list_cap 0); nq, q_stride, nkf_rows, cap or nmp < 1; nobs or list_cap < 0.  ORBM_E_CAPACITY: nq > ORBM_COVIS_MAX_QUERIES,
 * q_stride > ORBM_COVIS_MAX_SLOTS, nkf_rows > ORBM_COVIS_MAX_ROWS, nmp > ORBM_MP_MAX_BATCH, nq * nkf_rows > ORBM_COVIS_MAX_VOTES,
 * nkf_rows * cap > 2^31 - 1.  No CPU fallback: ORBM_E_HIP without a device.
 *
 * orbm_local_points (host pointers, synchronous) / orbm_local_points_batch_async (device pointers, enqueue-only): one parameter list.
 * lkf_row [T][lkf_stride], n_lkf [T] = per frame the local KeyFrames' pool rows IN THE ORDER WALKED: the reference walks
 * mvpLocalKeyFrames with a reverse iterator (:3921), so the caller lays the list out reversed.  min(n_lkf, lkf_stride) rows are read, a
 * negative count reads as 0, a row outside [0, nkf_rows) contributes nothing.  kf_mp [nkf_rows][cap] is pool-wide: per pool slot the
 * MapPoint index of GetMapPointMatches()[i]; an index outside [0, nmp) means NULL.  mp_valid as above.
 * Semantics, for one frame.  Position (k, i) holds the MapPoint j = kf_mp[lkf_row[k]][i], for i < min(counts_kf[row], cap).  j is
 * emitted at its FIRST position in (k, i) lexicographic order, provided it is valid: the mnTrackReferenceForFrame test of :3938-3944.
 * A KeyFrame listed twice emits nothing the second time.
 * Outputs.  local_mp [T][q_stride] = the emitted indices in position order, which is the order of mvpLocalMapPoints (M3's claim
 * order); n_total [T] = how many MapPoints were emitted in all; nq [T] = min(n_total, q_stride).  Emissions beyond q_stride are
 * dropped; slots at and beyond nq keep the caller's bytes.  local_mp and nq are inputs of orbm_gather_map_points_batch_async and
 * orbm_is_in_frustum_batch_async.  Both forms return ORBM_OK.
 * Scratch: the first positions [T][nmp] and the chunk counts are handle-owned, grown by an eager call; after one eager call the same
 * or a smaller shape enqueues with no allocation and can be captured (orbx_capture_begin).  The first positions are reset by a memset
 * inside the enqueued work.
 * ORBM_E_INVALID, with nothing enqueued: a NULL array (mp_valid may be NULL); T, lkf_stride, nkf_rows, cap, nmp or q_stride < 1.
 * ORBM_E_CAPACITY: T > ORBM_LOCALPTS_MAX_FRAMES, lkf_stride > ORBM_LOCALPTS_MAX_KFS, cap > ORBM_LOCALPTS_MAX_CAP, lkf_stride * cap >
 * 2^31 - 1, T * nmp > ORBM_COVIS_MAX_VOTES, nmp > ORBM_MP_MAX_BATCH.  ORBM_E_HIP without a device.
 *
 * orbm_gather_map_points_batch_async (device pointers, enqueue-only; there is no host form): for e < min(nq[f], q_stride) and j =
 * local_mp[f][e] the MapPoint pool rows mp_pw [nmp][3], mp_normal [nmp][3], mp_min_dist, mp_max_dist [nmp], mp_desc [nmp][32] and
 * mp_nobs [nmp] (int32, Observations()) are copied to pw, normal [T][q_stride][3], min_dist, max_dist [T][q_stride], qdesc
 * [T][q_stride][32] and mp_obs [T][q_stride] (uint8, mp_nobs > 0): the rows orbm_is_in_frustum_batch_async and
 * orbm_search_by_projection_points_batch_async read.  skip [T][q_stride] = mp_skip [T][nmp] at j, the caller's mnLastFrameSeen == mnId
 * flags; with mp_skip NULL it is 0.  Every source / destination pair is optional: a NULL destination (or source) is not written.
 * Entries at and beyond nq[f] keep the caller's bytes.  An index outside [0, nmp), possible only if the caller wrote local_mp itself,
 * gets skip = 1 and nothing else.  Alignment: mp_desc and qdesc must be 16-byte aligned (descriptor rows move as two 128-bit words);
 * every other array is aligned to its element.  No scratch; capturable from the first call.  ORBM_E_INVALID: local_mp or nq NULL; T,
 * q_stride or nmp < 1; a misaligned descriptor array.  ORBM_E_CAPACITY: T > ORBM_LOCALPTS_MAX_FRAMES, nmp > ORBM_MP_MAX_BATCH. */
enum { ORBM_COVIS_MAX_QUERIES = 65535, ORBM_COVIS_MAX_SLOTS = 65535, ORBM_COVIS_MAX_ROWS = 1 << 20, ORBM_COVIS_MAX_VOTES = 1 << 28 };
enum { ORBM_LOCALPTS_MAX_FRAMES = 65535, ORBM_LOCALPTS_MAX_KFS = 65535, ORBM_LOCALPTS_MAX_CAP = 65535 };
int orbm_covisibility_votes(orbm_t*, int nq, int q_stride, const int32_t* q_mp, const int32_t* q_n, const int32_t* self_row,
                            int nkf_rows, int cap, const int32_t* counts_kf, const uint8_t* kf_skip, int skip_bad,
                            int nmp, int nobs, const int32_t* obs_off, const int32_t* obs_row, const int32_t* obs_slot,
                            const uint8_t* obs_flags, const uint8_t* mp_valid, int th, int list_cap,
                            int32_t* votes, int32_t* n_voted, int32_t* max_votes, int32_t* n_over, int32_t* list_row, int32_t* list_votes);
int orbm_covisibility_votes_batch_async(orbm_t*, int nq, int q_stride, const int32_t* q_mp, const int32_t* q_n, const int32_t* self_row,
                                        int nkf_rows, int cap, const int32_t* counts_kf, const uint8_t* kf_skip, int skip_bad,
                                        int nmp, int nobs, const int32_t* obs_off, const int32_t* obs_row, const int32_t* obs_slot,
                                        const uint8_t* obs_flags, const uint8_t* mp_valid, int th, int list_cap,
                                        int32_t* votes, int32_t* n_voted, int32_t* max_votes, int32_t* n_over, int32_t* list_row, int32_t* list_votes);
int orbm_local_points(orbm_t*, int T, int lkf_stride, const int32_t* lkf_row, const int32_t* n_lkf, int nkf_rows, int cap,
                      const int32_t* counts_kf, const int32_t* kf_mp, int nmp, const uint8_t* mp_valid, int q_stride,
                      int32_t* local_mp, int32_t* n_total, int32_t* nq);
int orbm_local_points_batch_async(orbm_t*, int T, int lkf_stride, const int32_t* lkf_row, const int32_t* n_lkf, int nkf_rows, int cap,
                                  const int32_t* counts_kf, const int32_t* kf_mp, int nmp, const uint8_t* mp_valid, int q_stride,
                                  int32_t* local_mp, int32_t* n_total, int32_t* nq);
int orbm_gather_map_points_batch_async(orbm_t*, int T, int q_stride, const int32_t* local_mp, const int32_t* nq, int nmp,
                                       const float* mp_pw, const float* mp_normal, const float* mp_min_dist, const float* mp_max_dist,
                                       const uint8_t* mp_desc, const int32_t* mp_nobs, const uint8_t* mp_skip,
                                       float* pw, float* normal, float* min_dist, float* max_dist, uint8_t* qdesc, uint8_t* mp_obs, uint8_t* skip);

/* ---- Pose optimisation on the device: Optimizer::PoseOptimization(Frame*) (Optimizer.cc:943-1286) for !pFrame->mpCamera2 -- pinhole,
 * Nleft == -1, monocular (mvuRight < 0) and stereo edges in one frame -- and the bookkeeping Tracking wraps around it: the outlier discard
 * loops (Tracking.cc:3029-3059, :3239-3266), mnMatchesInliers (:3388-3410) and step 1 of SearchLocalPoints (:3812-3832).  Nothing else
 * of Optimizer.cc is here; the mpCamera2 branch (:1085-1152), other camera models and the inertial optimisations stay with the caller.
 * This is the one entry point whose result is held to a TOLERANCE against the reference and not to bits: g2o sums in Eigen's order
 * on the host's FMA unit and holds the rotation as a quaternion.  Against this library's own arithmetic (csrc/orbm_poseopt.h, which
 * the host tests compile) the device result is bit-identical, pose included.
 *
 * orbm_pose_optimization (host pointers, synchronous) / orbm_pose_optimization_batch_async (device pointers except k_host and
 * inv_level_sigma2_host, enqueue-only): one parameter list, one kernel.
 * Rows.  Frame f of the call is block frame first + f of kps_un (mvKeysUn) and counts, rows of cap slots, as
 * orbm_unproject_stereo_batch_async takes them; min(max(counts, 0), cap) slots are read.  uright [nframes][cap] = mvuRight, or NULL: every
 * edge is mono.  q_mp [nframes][cap] = the frame's mvpMapPoints as indices into the MapPoint pool, an index outside [0, nmp) is NULL (the
 * convention of orbm_covisibility_votes_batch_async); mp_pw [nmp][3] = the pool's world positions (orbm_gather_map_points_batch_async).
 * tcw_in / tcw_out [nframes][12] = the row-major 3x4 [Rcw | tcw] of orbm_is_in_frustum_batch_async, DEVICE rows in the async form, so a
 * replayed graph follows new poses and new match rows; tcw_out == tcw_in is allowed (SetPose).  k_host = (fx, fy, cx, cy), bf = mbf,
 * inv_level_sigma2_host [nlevels] = mvInvLevelSigma2 hold for every frame of the call.  A slot whose octave is outside [0, nlevels) is
 * treated as NULL (the reference would read past mvInvLevelSigma2).
 * The rules, each restated in csrc/orbm_poseopt.h with its citation:
 *  - edges: one per slot with a MapPoint, in slot order; information = inv_level_sigma2[octave] * I; Huber delta (float)sqrt(5.991) for a
 *    mono and (float)sqrt(7.815) for a stereo edge, widened to double; no isBad() test.
 *  - the < 3 rule: with fewer than 3 edges nothing is optimised: n_good = 0, the flags of the slots that hold a MapPoint are cleared and
 *    tcw_out[f] = tcw_in[f], bit for bit.
 *  - the float invz: the stereo error uses cam_project's `const float invz = 1.0f / z` (the double quotient rounded to float), the
 *    stereo Jacobian the double invz, as types_six_dof_expmap.cpp:339-404 writes them; the mono error is obs - (fx * x / z + cx, ...).
 *  - Levenberg-Marquardt as optimization_algorithm_levenberg.cpp:61-194 with the dense LDLT and SE3Quat::exp, both theta branches; at
 *    most 10 iterations of at most 10 trials per round.
 *  - the round-restart rule: four rounds, and EVERY round starts from the input pose (Optimizer.cc:1176 reads mTcw, which is written
 *    after the last round only); the rounds differ in their active set and, in the last, in having no robust kernel.
 *  - classification after each round: (float)chi2 > 5.991f / 7.815f, strictly; an edge flagged as an outlier is recomputed at the round's
 *    final pose.  The stale-error rule: an inlier edge is read as the last computeActiveErrors left it, which after a rejected last
 *    trial is the error at the REJECTED pose (pop() restores the estimate, not the errors).
 *  - the < 10 rule: with fewer than 10 edges in all (active or not) only the first round runs.  A round with an empty active set
 *    leaves the estimate at the input pose and classifies there.
 *  - the reduction order: slot s belongs to thread s % 256 and a thread adds its slots in ascending order; the 64 lanes of a wave
 *    combine by an xor butterfly (masks 32 ... 1), the four wave sums are added in wave order.  It is part of the contract: it fixes
 *    the bits, and csrc/orbm_poseopt.h replays it on the host.
 * Outputs.  outlier [nframes][cap] = mvbOutlier, written ONLY for slots that hold a MapPoint (the others keep the caller's bytes); n_corr
 * [nframes] = nInitialCorrespondences; n_good [nframes] = the return value, nInitialCorrespondences - nBad of the last round run; tcw_out
 * = the estimate rounded to float (Converter::toCvMat).  Both forms return ORBM_OK.
 * The device form is ONE launch of one workgroup per frame: all four rounds, their iterations and trials run inside it with data-dependent
 * loops; no host decision, no scratch, no atomics, nothing accumulates across replays: capturable (orbx_capture_begin) from the first call.
 * With cap <= 1536 the frame's edges are staged in LDS once; a larger cap gathers them from the rows in every pass (same bits, slower).
 * ORBM_E_INVALID, with nothing enqueued: a NULL array other than uright; nframes, cap, nmp or nlevels < 1; first < 0; a k_host entry or bf
 * that is not finite.  ORBM_E_CAPACITY: nframes > ORBM_POSEOPT_MAX_FRAMES, cap > ORBM_POSEOPT_MAX_CAP, nlevels > ORBM_POSEOPT_MAX_LEVELS, nmp >
 * ORBM_MP_MAX_BATCH, (first + nframes) * cap > 2^31 - 1.  No CPU fallback: ORBM_E_HIP without a device.
 *
 * orbm_discard_outliers_batch_async (device pointers, enqueue-only; there is no host form): counts [nframes], q_mp and outlier
 * [nframes][cap] are the rows above (counts already offset by first), both IN/OUT; mp_nobs [nmp] = Observations(), mp_valid [nmp] = !isBad()
 * (NULL = all valid).  For slot i < min(max(counts[f], 0), cap) with a MapPoint j = q_mp[f][i] inside [0, nmp):
 *  - with discard != 0 and outlier[f][i] set (Tracking.cc:3038-3054): q_mp = -1, outlier = 0, mp_seen[f][j] = 1 (mnLastFrameSeen), and the
 *    slot is counted in n_discarded[f];
 *  - otherwise n_matches_map[f] counts the slot if it is not an outlier and mp_nobs[j] > 0 (:3055-3057; mnMatchesInliers of :3388-3410 with
 *    discard == 0); then, with clear_bad != 0 and mp_valid[j] == 0, the slot becomes -1 (:3817-3819), else mp_seen[f][j] = 1 (:3826).
 * mp_seen [nframes][nmp] is the mp_skip row of orbm_gather_map_points_batch_async; it is zeroed inside the enqueued work and takes plain
 * byte stores of the value 1 (several slots may hit one MapPoint).  The two count rows are zeroed there too and summed by ballot popcount
 * and one integer atomic per wave: exact, and the same on every replay.  mp_seen, n_matches_map and n_discarded may each be NULL (not
 * wanted).  No scratch; capturable from the first call.  ORBM_E_INVALID: counts, q_mp, outlier or mp_nobs NULL; nframes, cap or nmp < 1.
 * ORBM_E_CAPACITY: nframes > ORBM_POSEOPT_MAX_FRAMES, cap > ORBM_POSEOPT_MAX_CAP, nmp > ORBM_MP_MAX_BATCH, nframes * nmp > 2^28. */
enum { ORBM_POSEOPT_MAX_FRAMES = 65535, ORBM_POSEOPT_MAX_CAP = 65535, ORBM_POSEOPT_MAX_LEVELS = 32 };
int orbm_pose_optimization(orbm_t*, int nframes, int first, int cap, const orbm_kp_t* kps_un, const int32_t* counts,
                           const float* uright, const int32_t* q_mp, int nmp, const float* mp_pw, const float* tcw_in,
                           const float* k_host, float bf, const float* inv_level_sigma2_host, int nlevels,
                           float* tcw_out, uint8_t* outlier, int32_t* n_corr, int32_t* n_good);
int orbm_pose_optimization_batch_async(orbm_t*, int nframes, int first, int cap, const orbm_kp_t* kps_un, const int32_t* counts,
                                       const float* uright, const int32_t* q_mp, int nmp, const float* mp_pw, const float* tcw_in,
                                       const float* k_host, float bf, const float* inv_level_sigma2_host, int nlevels,
                                       float* tcw_out, uint8_t* outlier, int32_t* n_corr, int32_t* n_good);
int orbm_discard_outliers_batch_async(orbm_t*, int nframes, int cap, const int32_t* counts, int32_t* q_mp, uint8_t* outlier,
                                      int nmp, const int32_t* mp_nobs, const uint8_t* mp_valid, int discard, int clear_bad,
                                      uint8_t* mp_seen, int32_t* n_matches_map, int32_t* n_discarded);

/* ---- CreateNewMapPoints behind M10: step 6 of LocalMapping::CreateNewMapPoints (LocalMapping.cc:609-892) for every match M10 left in
 * matches12 -- the parallax tests, the linear triangulation or UnprojectStereo_, the two reprojection tests, the scale-consistency test, the
 * cross-pair rule and the order in which the reference creates its MapPoints.  Pinhole cameras, NLeft == -1, !mpCamera2; the
 * baseline / median-depth tests (:552-578) stay with the caller: a pair that fails them is simply not passed.  new MapPoint, AddObservation and
 * AddMapPoint stay with the caller too, who walks `order`.
 * x3d is held to a TOLERANCE against the reference and is NOT bit-identical to cv::SVD: the null vector of the 4x4 (:768) comes from a
 * one-sided Jacobi in float32 (csrc/orbm_triangulate.h), whose sign-aligned unit vector lies within C * eps32 * sigma1 / (sigma3 - sigma4) of
 * the float64 one (C and its measurement: tests/triangulate_results.py, profiles/NOTES.md).  On the UnprojectStereo_ branches there is no SVD
 * and x3d is the reference's float expression.  Against this library's own arithmetic (the header, which the host tests compile) the device
 * result is bit-identical, x3d included.
 *
 * orbm_triangulate_new_points_batch_async (device pointers except group_start_host and the *_host tables, enqueue-only) /
 * orbm_triangulate_new_points (the same list behind `space`: ORBM_HOST = every array is a host array, ORBM_DEVICE = device arrays as in the
 * async form; synchronous in both): one parameter list, the same two kernels.
 * Groups.  Group g is ONE current KeyFrame: its pairs are [group_start_host[g], group_start_host[g + 1]), they share one row1 and are walked
 * in the order given (the order of vpNeighKFs).  group_start_host [ngroups + 1] is a HOST array in both forms, runs from 0 to npairs and is
 * copied into the launch (a captured graph keeps it).  A group whose pairs do not share one row1 is refused: ORBM_E_INVALID where row1 is
 * readable (ORBM_HOST); in the device forms such a group creates nothing and its reason rows read 15.
 * Pools as in orbm_search_for_triangulation_batch_async: pool 1 has nrows1 rows of cap1 slots -- kps_un1 (mvKeysUn), kps1 (mvKeys, read only
 * by UnprojectStereo_; NULL = kps_un1), counts1 [nrows1], uright1 (mvuRight; NULL = no stereo feature), depth1 (mvDepth; NULL = -1), tcw1
 * [nrows1][12] = the row-major 3x4 [Rcw | tcw], ow1 [nrows1][3] = GetCameraCenter --, pool 2 the same with nrows2 / cap2; one pool may be
 * passed twice.  row1 / row2 [npairs] and matches12 [npairs][cap1] are M10's arrays as they are.  k1_host / k2_host = (fx, fy, cx, cy,
 * invfx, invfy) of the current KeyFrames / the neighbours, mb1 / mbf1 = the current KeyFrame's mb / mbf, mb2 = the neighbours' mb;
 * scale_factors*_host = mvScaleFactors, level_sigma2_*_host = mvLevelSigma2 [nlevels]; ratio_factor = 1.5f * mfScaleFactor; th_far =
 * mThFarPoints, <= 0: mbFarPoints is off.
 * The rules, each restated in csrc/orbm_triangulate.h with its citation:
 *  - a match is idx2 = matches12[p][idx1] with idx1 < the row-1 count and 0 <= idx2 < the row-2 count; anything else in the entry (-1,
 *    garbage below -1 or past the count) and a row1 / row2 outside its pool read as "no match" and are never dereferenced.
 *  - bStereo = uright >= 0; `if (bStereo1) ... else if (bStereo2)` as written: cosParallaxStereo2 is computed only when KeyFrame 1's feature
 *    is not stereo; cos(2 * atan2(mb / 2, depth)) in double, stored to float.
 *  - triangulate when cosParallaxRays < cosParallaxStereo, > 0 and (either feature stereo or < 0.9998); else UnprojectStereo_ of KeyFrame 1,
 *    else of KeyFrame 2 (mvKeys; zeros for depth <= 0), else reject.  x3D_h(3) == 0 rejects.
 *  - z1 <= 0, z2 <= 0 reject; invz = 1.0 / z stored to float; mono error through project() (fx * x / z + cx), stereo error fx * x * invz + cx.
 *    The mbf1 rule: u2_r of the SECOND KeyFrame subtracts mbf1 * invz2 -- KeyFrame 1's mbf, as :861 reads mpCurrentKeyFrame->mbf.
 *    chi2 > 5.991 * sigma2 (mono) / > 7.8 * sigma2 (stereo) against the double product.
 *  - dist == 0 rejects; with th_far > 0, dist >= th_far rejects; ratioDist * ratio_factor < ratioOctave || ratioDist > ratioOctave *
 *    ratio_factor rejects.  An octave outside [0, nlevels) rejects and indexes no table.
 *  - the cross-pair rule: per idx1 the pairs of the group are tried in order and the FIRST pair whose match passes every gate wins; a later
 *    pair's match for that idx1 is dropped (reason 4), as the reference's search of a later neighbour skips a feature that already holds a
 *    MapPoint.  A pair whose match fails leaves idx1 free for the next pair.
 * Outputs.  won_pair [ngroups][cap1] = the winning pair's index in [0, npairs) or -1, won_idx2 = its idx2 or -1, x3d [ngroups][cap1][3] =
 * the new point (zeros where won_pair is -1); reason [npairs][cap1] (optional, NULL = not wanted) = the exit of every (pair, idx1), the
 * values of enum TriReason in csrc/orbm_triangulate.h (0..2 success by branch, 3 no match, 4 taken by an earlier pair, 5..14 the gates);
 * ncreated [npairs] = the MapPoints pair p creates; order [ngroups][cap1] = the group's winning idx1 in the reference's creation order (pair
 * by pair, ascending idx1 inside a pair), -1 past ntotal [ngroups].  Every slot of every output row is written by every call; counts start
 * from zero inside the enqueued work, nothing is atomic, a replayed graph repeats its result.  No scratch, no allocation: capturable
 * (orbx_capture_begin) from the first call.  Both forms return ORBM_OK.
 * ORBM_E_INVALID, with nothing enqueued: a NULL array other than kps1 / kps2, uright*, depth* and reason; ngroups, npairs, nrows*, cap* or
 * nlevels < 1; group_start_host not starting at 0, not ending at npairs or not monotone; a ratio_factor that is not finite; a `space` that is
 * neither.  ORBM_E_CAPACITY: cap1 or cap2 > ORBM_TRI_MAX_CAP, npairs > ORBM_TRI_MAX_PAIRS, a group of more than ORBM_TRI_MAX_GROUP_PAIRS pairs,
 * nlevels > ORBM_TRI_MAX_LEVELS.  No CPU fallback: ORBM_E_HIP without a device. */
enum { ORBM_TRI_MAX_CAP = 65535, ORBM_TRI_MAX_PAIRS = 65535, ORBM_TRI_MAX_GROUP_PAIRS = 64, ORBM_TRI_MAX_LEVELS = 32 };
int orbm_triangulate_new_points_batch_async(orbm_t*, int ngroups, const int32_t* group_start_host, int npairs,
                                            int nrows1, int cap1, const orbm_kp_t* kps_un1, const orbm_kp_t* kps1, const int32_t* counts1,
                                            const float* uright1, const float* depth1, const float* tcw1, const float* ow1,
                                            int nrows2, int cap2, const orbm_kp_t* kps_un2, const orbm_kp_t* kps2, const int32_t* counts2,
                                            const float* uright2, const float* depth2, const float* tcw2, const float* ow2,
                                            const int32_t* row1, const int32_t* row2, const int32_t* matches12,
                                            const float* k1_host, const float* k2_host, float mb1, float mbf1, float mb2,
                                            const float* scale_factors1_host, const float* level_sigma2_1_host,
                                            const float* scale_factors2_host, const float* level_sigma2_2_host,
                                            int nlevels, float ratio_factor, float th_far,
                                            int32_t* won_pair, int32_t* won_idx2, float* x3d, uint8_t* reason, int32_t* ncreated,
                                            int32_t* order, int32_t* ntotal);
int orbm_triangulate_new_points(orbm_t*, int space, int ngroups, const int32_t* group_start_host, int npairs,
                                int nrows1, int cap1, const orbm_kp_t* kps_un1, const orbm_kp_t* kps1, const int32_t* counts1,
                                const float* uright1, const float* depth1, const float* tcw1, const float* ow1,
                                int nrows2, int cap2, const orbm_kp_t* kps_un2, const orbm_kp_t* kps2, const int32_t* counts2,
                                const float* uright2, const float* depth2, const float* tcw2, const float* ow2,
                                const int32_t* row1, const int32_t* row2, const int32_t* matches12,
                                const float* k1_host, const float* k2_host, float mb1, float mbf1, float mb2,
                                const float* scale_factors1_host, const float* level_sigma2_1_host,
                                const float* scale_factors2_host, const float* level_sigma2_2_host,
                                int nlevels, float ratio_factor, float th_far,
                                int32_t* won_pair, int32_t* won_idx2, float* x3d, uint8_t* reason, int32_t* ncreated,
                                int32_t* order, int32_t* ntotal);

/* M15 Frame::ComputeStereoMatches (Frame.cc:1027-1276).  left/right are orbx_t* extractor handles (include/orbx.h)
 * on the same device whose LAST call produced the two keypoint sets: their device-resident pyramids supply the
 * 11x11 SAD windows (mvImagePyramid, include/ORBextractor.h:83).  frame_l/frame_r select the batch slot.
 * uright/depth: host outputs [nl] (mvuRight, mvDepth).  Returns the number of stereo points kept. */
int orbm_stereo_matches(orbm_t*, void* left_extractor, int frame_l, void* right_extractor, int frame_r,
                        int nl, const orbm_kp_t* kl, const uint8_t* dl, int nr, const orbm_kp_t* kr, const uint8_t* dr,
                        float mb, float mbf, float* uright, float* depth);

/* SURVEY 8(f).2  Frame::UndistortKeyPoints (Frame.cc:924-970): cv::undistortPoints(points, K, D, R = I, P = newK) on the
 * coordinates of n keypoints (other fields copied).  k / newk = (fx, fy, cx, cy); dist = (k1, k2, p1, p2[, k3 ...]),
 * ndist <= 14 in OpenCV's order (k1, k2, p1, p2, k3, k4, k5, k6, s1, s2, s3, s4, tauX, tauY): the radial, tangential, rational
 * and thin-prism terms are applied.  The tilted sensor model is NOT implemented: a call whose dist[12] or dist[13] is nonzero is
 * refused with ORBM_E_INVALID (orbm_last_error says so) before anything is launched -- the reference never passes more than five
 * coefficients (Frame.cc:924-970).  dist[0] == 0 copies the input (Frame.cc:928-932).  space = ORBM_HOST | ORBM_DEVICE for kps
 * and out. */
int orbm_undistort_keypoints(orbm_t*, int space, const orbm_kp_t* kps, int n, const float* k, const float* dist, int ndist,
                             const float* newk, orbm_kp_t* out);
/* Frame::ComputeImageBounds (Frame.cc:977-1021): bounds[4] = (mnMinX, mnMaxX, mnMinY, mnMaxY) (host output).  Nonzero tilt
 * coefficients are refused as above. */
int orbm_image_bounds(orbm_t*, int cols, int rows, const float* k, const float* dist, int ndist, const float* newk, float* bounds);

/* SURVEY 8(f).3  Frame::isInFrustum (Nleft == -1; Frame.cc:603-671) + MapPoint::PredictScale (MapPoint.cc:725-740) +
 * Pinhole::project for n map points: the producer of the arrays orbm_search_by_projection_points consumes.
 * pw / normal: [n][3] world position and mean viewing direction; min_dist / max_dist: mfMinDistance / mfMaxDistance;
 * rcw[9] row-major, tcw[3], ow[3]; k = (fx, fy, cx, cy); bounds = (minX, maxX, minY, maxY); bf = mbf.
 * Outputs mirror the MapPoint members: in_view (mbTrackInView), proj_x / proj_y (mTrackProjX/Y, -1 unless the point
 * passed the image-bounds test), proj_xr, depth (mTrackDepth), level (mnTrackScaleLevel), view_cos -- the last four are
 * written only where in_view.  All arrays in `space`.  Returns the number of points in view (host space) or 0. */
int orbm_is_in_frustum(orbm_t*, int space, int n, const float* pw, const float* normal, const float* min_dist, const float* max_dist,
                       const float* rcw, const float* tcw, const float* ow, const float* k, const float* bounds,
                       float bf, float viewing_cos_limit, float log_scale_factor, int n_scale_levels,
                       uint8_t* in_view, float* proj_x, float* proj_y, float* proj_xr, float* depth, int32_t* level, float* view_cos);
/* orbm_is_in_frustum_batch_async: the loop of Tracking::SearchLocalPoints (Tracking.cc:3808-3862) over Frame::isInFrustum for `nframes`
 * frames in ONE launch, with everything that changes from frame to frame read from device rows: the producer of the query rows of
 * orbm_search_by_projection_points_batch_async, written in place.  Frame f's pose is tcw [nframes][12], the row-major 3x4 [Rcw | tcw]
 * (mRcwx, mtcwx; the layout of orbm_search_by_projection_kf_batch_async and orbm_fuse_batch_async), and ow [nframes][3] (mOwx); its point
 * count is nq[f], used as min(max(nq[f], 0), q_stride).  The MapPoint rows pw / normal [..][q_stride][3] and min_dist / max_dist
 * [..][q_stride] are [nframes] rows, or ONE row for every frame -- the same local map -- when q_shared != 0.  k_host = (fx, fy, cx, cy)
 * and bounds_host = (minX, maxX, minY, maxY) are host pointers and, like bf, viewing_cos_limit, log_scale_factor and n_scale_levels, hold
 * for every frame of the call.  Arithmetic, order of the gates and level rule are those of orbm_is_in_frustum: both forms run one device
 * function and give the same bits.
 * Skip rule: skip [nframes][q_stride] (always per frame; NULL = none) is step 1 of SearchLocalPoints, set by the caller to
 * `pMP->mnLastFrameSeen == frame.mnId || pMP->isBad()`: a point already matched in the frame (:3844) or bad (:3847).  An entry with
 * skip != 0 gets in_view = 0 and NOTHING ELSE of it is written -- the reference sets mbTrackInView = false (:3828) and leaves mTrackProjX/Y alone, and
 * it never searches a bad point whatever its stale flag (ORBmatcher.cc:45-80).
 * Tail rule: entries nq[f] <= i < q_stride get in_view = 0 and their other six fields are not written.
 * Outputs, rows [nframes][q_stride] of the seven arrays orbm_search_by_projection_points_batch_async takes (depth is its th_far row): for a
 * point that is neither skipped nor in the tail in_view is written always; proj_x / proj_y are -1 unless the point passed the image-bounds
 * test and stay set when a later gate rejects it; proj_xr, depth, level and view_cos are written only where in_view == 1 -- a rejected
 * point keeps the caller's bytes there.
 * Count: n_in_view [nframes] (NULL = not wanted) = the number of entries of row f with in_view == 1, the reference's nToMatch (:3856).  It
 * is summed with integer atomics into a row that a memset inside the enqueued work zeroes first: exact, and the same on every replay.
 * All pointers are device pointers except k_host and bounds_host.  Enqueue-only, no scratch and no work buffer: the call can be captured
 * (orbx_capture_begin) from the first call, and a replayed graph follows new poses, counts and skip flags in the rows.  The fisheye
 * isInFrustum (Nleft != -1, KannalaBrandt8::project) stays with the caller.  ORBM_E_INVALID: a NULL required array (skip and n_in_view
 * may be NULL); nframes, q_stride or n_scale_levels < 1; a viewing_cos_limit or log_scale_factor that is not finite.  ORBM_E_CAPACITY:
 * nframes > 65535; q_stride > ORBM_LP_MAX_QUERIES.  Nothing is enqueued on either error and orbm_last_error names the argument.  A NULL
 * handle is ORBM_E_HIP where there is no device (no CPU fallback) and ORBM_E_INVALID otherwise.  Returns ORBM_OK. */
int orbm_is_in_frustum_batch_async(orbm_t*, int nframes, const float* tcw, const float* ow,
                                   const int32_t* nq, int q_stride, const uint8_t* skip,
                                   const float* pw, const float* normal, const float* min_dist, const float* max_dist, int q_shared,
                                   const float* k_host, const float* bounds_host, float bf, float viewing_cos_limit,
                                   float log_scale_factor, int n_scale_levels,
                                   uint8_t* in_view, float* proj_x, float* proj_y, float* proj_xr, float* depth, int32_t* level, float* view_cos,
                                   int32_t* n_in_view);

#ifdef __cplusplus
}
#endif
#endif
