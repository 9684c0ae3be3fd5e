/*
 * pbrhip.h -- C ABI of the MI355X-native path-tracing core that sits behind pbrlab's
 * Scene / Render() / RenderLayer API (libpbrhip.so, built from pbrlab_amd/csrc).
 *
 * This is the drop-in boundary: scene construction keeps pbrlab's builder calls,
 * BVH build/flatten and tile dispatch stay on the host inside the library, and the per-sample hot
 * path -- camera ray -> GetRadiance bounce loop -> RenderLayer accumulation -- runs as HIP kernels.
 * Plain pointers and sizes only; host pointers in, host pointers out unless a function says "device".
 * Every entry point cites the reference interface it replaces (file:line under lighttransport/pbrlab).
 *
 * All functions return 0 on success or a negative PBRHIP_E* code; pbrhip_last_error() returns a
 * thread-local message.  The library fails loudly (PBRHIP_ENODEVICE) when no HIP device is usable:
 * there is no CPU fallback.
 */
#ifndef PBRHIP_H_
#define PBRHIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PBRHIP_OK 0
#define PBRHIP_EINVAL (-1)    /* bad argument / id out of range */
#define PBRHIP_ESIZE (-2)     /* std::runtime_error("... param error") cases of scene.cc:64-94 */
#define PBRHIP_ENODEVICE (-3) /* no usable HIP device */
#define PBRHIP_EHIP (-4)      /* a HIP runtime call failed */
#define PBRHIP_EUNSUPPORTED (-5)
#define PBRHIP_ESTATE (-6)    /* scene not committed / already committed / stale (geometry edits pending: pbrhip_scene_refit) */
#define PBRHIP_EOVERFLOW (-7) /* traversal stack overflow (BVH deeper than the kernel supports) */
#define PBRHIP_ENOMEM (-8)    /* host allocation failed (std::bad_alloc) */
#define PBRHIP_ECOMM (-9)     /* RCCL is unavailable or one of its calls failed */

#define PBRHIP_NONE 0xFFFFFFFFu

typedef struct pbrhip_scene pbrhip_scene;

/* pbrlab::CyclesPrincipledBsdfParameter (src/material-param.h:24-49), name dropped */
typedef struct {
  float base_color[3];
  float subsurface;
  float subsurface_radius[3];
  float subsurface_color[3];
  float metallic, specular, specular_tint, roughness, anisotropic, anisotropic_rotation;
  float sheen, sheen_tint, clearcoat, clearcoat_roughness, ior, transmission, transmission_roughness;
  uint32_t base_color_tex_id, subsurface_color_tex_id; /* PBRHIP_NONE or an id from pbrhip_scene_add_texture */
} pbrhip_principled_param;

/* pbrlab::HairBsdfParameter (src/material-param.h:51-72) */
typedef struct {
  uint32_t coloring_hair; /* 0 = kRGB, 1 = kMelanin */
  float base_color[3];
  float melanin, melanin_redness, melanin_randomize;
  float roughness, azimuthal_roughness, ior, shift;
  float specular_tint[3], second_specular_tint[3], transmission_tint[3];
} pbrhip_hair_param;

/* pbrlab::Ray (src/ray.h:9-14), packed as two float4 */
typedef struct {
  float org[3];
  float tmin;
  float dir[3];
  float tmax;
} pbrhip_ray;

/* pbrlab::TraceResult (src/raytracer/raytracer.h:9-17) */
typedef struct {
  float normal_g[3];
  float t, u, v;
  uint32_t instance_id, geom_id, prim_id;
} pbrhip_hit;

/* arguments of pbrlab::Render (src/render.h:14-17) plus what the reference hard-wires */
typedef struct {
  uint32_t width, height, num_sample; /* Render(scene, width, height, num_sample, ...) */
  uint32_t first_pass;                /* passes [first_pass, first_pass+num_sample) (progressive resume) */
  uint64_t seed_seq;                  /* PCG32 initseq; the reference uses 1234567890 (render.cc:215) */
  uint32_t tile_rank, tile_world;     /* 64x64 tiles (render.cc:107-108) with index % world == rank */
  uint32_t max_paths_in_flight;       /* 0 = default (half of the free HBM, <= 256 Mi): passes are rendered in chunks of this many paths */
  uint32_t flags;                     /* PBRHIP_RENDER_* */
  uint32_t num_streams;               /* the passes of a chunk are split into path groups, one HIP stream each (pbrhip.cpp::plan_groups).
                                         0 = default: two equal groups started at once when the chunk holds at least 96 Mi paths,
                                         otherwise one (pipelined plans were measured and lost); n > 0: n equal groups (at most 16),
                                         of which at most 8 are in flight at a time */
  uint32_t tail_paths;                /* once a group has at most this many live paths, the rest of every path runs in ONE launch
                                         (k_tail) instead of one set of launches per bounce; 0 = default 262144, 0xFFFFFFFF = never */
  uint32_t shard_block;               /* edge of the square pixel blocks dealt to ranks (block index % tile_world == tile_rank);
                                         0 = 64, the reference's tile (render-tile.cc:29-41).  Smaller blocks balance the load of
                                         many GPUs better; the image does not depend on it */
} pbrhip_render_desc;

#define PBRHIP_RENDER_STATS 1u   /* count BVH nodes / primitives visited (slower; for algorithmic bytes) */
#define PBRHIP_RENDER_TIMING 2u  /* time every kernel launch with HIP events on the render stream */
#define PBRHIP_RENDER_NO_CLEAR 4u /* keep the layer's current contents (Render() clears: render.cc:99-100) */
#define PBRHIP_RENDER_TIMING_TRACE 8u /* time only the k_trace launches (ms_trace_closest / n_trace_closest): a sixth of the events of
                                         PBRHIP_RENDER_TIMING, for measurements that must not slow the frame (bench.py's timed region) */

/* filled by pbrhip_render when stats != NULL */
typedef struct {
  uint64_t samples, iterations, chunks;
  uint64_t closest_rays, closest_nodes, closest_tris, closest_curves; /* PBRHIP_RENDER_STATS */
  uint64_t shadow_rays, shadow_nodes, shadow_tris, shadow_curves;
  /* PBRHIP_RENDER_TIMING: total ms and launch count per kernel */
  double ms_generate, ms_trace_closest /* = k_trace: closest + shadow rays */, ms_surface /* = k_classify */, ms_shade_principled, ms_shade_hair, ms_sss_step,
      ms_tail /* = k_tail */, ms_accumulate, ms_compact;
  uint64_t n_trace_closest, n_tail, n_surface, n_shade_principled, n_shade_hair, n_sss_step;
  double ms_total; /* wall time of the call measured on the host */
  uint64_t tail_closest_rays, tail_shadow_rays; /* PBRHIP_RENDER_STATS: rays traced inside k_tail (not part of the k_trace counts above) */
  uint64_t pruned_rays; /* PBRHIP_RENDER_STATS: closest-hit rays of the reference that were never traced: the path's next
                           Russian roulette was already known to fail and the ray cannot reach an area light (it misses every
                           light primitive, or the bounding box of every light), so nothing it could find changes the image (closest + tail_closest + pruned = the reference's count) */
  uint64_t passes_done; /* passes every pixel of this rank holds when the call returns (= num_sample unless cancelled) */
  uint64_t node_bytes;  /* footprint of one node of the tree k_trace walked: 64 (the Q tree: 4 children, quantised boxes; or the binary tree) */
  uint64_t curve_bytes; /* bytes fetched per curve-piece test: 32 (Q tree: the two 16-byte end points of a piece in a curve record) or 64 (binary tree: one slot) */
  uint64_t suspended_rays; /* PBRHIP_RENDER_STATS: closest-hit rays a k_trace launch suspended at its drain and the next launch resumed
                              (counted ONCE in closest_rays; their node / primitive counts are complete: nothing is traversed twice) */
  double ms_host_idle;  /* PBRHIP_RENDER_TIMING: sum over the path groups of the time their stream sat empty between two bursts of
                           launches (the host's round trips; 0 when the next iteration was always enqueued in time) */
} pbrhip_render_stats;

/* The per-light shaft grid (PBRHIP_SHADOW_GRID=N cells per axis, 0 = off): shadow rays that start in a CLEAR cell
 * are answered by testing the few triangle leaves the cell lists instead of being traced.  pbrhip_render_stats keeps its layout, so what
 * the grid did is reported here: the three ray counters are those of the scene's last PBRHIP_RENDER_STATS render, which counts the rays
 * the grid answers and traces them all the same (shadow_rays, shadow_nodes, shadow_tris stay what they were without a grid). */
typedef struct {
  uint32_t resolution, num_lights, max_list; /* 0, 0, 0: the scene has no grid (more than 8 lights or none, curves, no Q tree, a transformed light, the knob) */
  uint32_t pad;
  uint64_t bytes;                            /* of device memory (part of pbrhip_scene_info's device_bytes) */
  uint64_t clear_cells, unknown_cells, empty_cells, listed_leaves; /* over all lights; empty_cells: CLEAR with an empty list */
  uint64_t culled_shadow_rays;               /* shadow rays the grid answers "unoccluded" (<= shadow_rays) */
  uint64_t clear_cell_rays, leaf_tests;      /* shadow rays that started in a CLEAR cell; two-triangle leaf tests made for them */
  double build_ms;                           /* the device build of the grid the scene holds */
} pbrhip_shadow_grid_info;
int pbrhip_scene_shadow_grid_info(pbrhip_scene*, pbrhip_shadow_grid_info* out);
/* the cells as the kernels read them (tests): num_lights x resolution^3 records of 8 words: count or 0xFFFFFFFF (UNKNOWN), then 7 leaf indices */
int pbrhip_scene_read_shadow_grid(pbrhip_scene*, uint32_t* cells, size_t num_words);

/* Layout version of the structs of this header (pbrhip_render_desc, pbrhip_render_stats, pbrhip_*_param, pbrhip_hit): it
 * changes whenever one of them changes (3 -> 4: pbrhip_render_stats grew by curve_bytes; 5 -> 6: by suspended_rays, ms_host_idle).  The library writes whole structs
 * (n of them for pbrhip_render_multi), so a caller compiled against another version must not call it: check
 * pbrhip_abi_version() == PBRHIP_ABI_VERSION once after loading (include/pbrlab_hip.hpp and pbrlab_amd/api.py do). */
#define PBRHIP_ABI_VERSION 6u
uint32_t pbrhip_abi_version(void);
/* Which implementation of cos / sin / exp / log -- the reference's std::cos ... on float, sampler/sampling-utils.h:10-14,
 * closure/microfacet-ggx.h:55-118, shader/random-walk-sss.h:116,183,192-194 -- this build of the library computes with:
 * PBRHIP_MATH_GLIBCF: GNU libc's float functions restated bit for bit (include/pbr_glibcf.h; the default since round 5: the
 * reference's own arithmetic where its libm is glibc 2.35 as Ubuntu 22.04 builds it, x86-64 with FMA: tests/test_glibcf.py); PBRHIP_MATH_F64R: the double-precision value
 * rounded once (include/pbr_f64r.h; a library built with -DPBR_MATH_F64R). */
#define PBRHIP_MATH_F64R 1u
#define PBRHIP_MATH_GLIBCF 2u
uint32_t pbrhip_math_mode(void);
size_t pbrhip_sizeof_render_stats(void); /* == sizeof(pbrhip_render_stats) of the library's build */

const char* pbrhip_last_error(void);
int pbrhip_device_count(int* count);
/* selects the HIP device used by subsequently created scenes (one process per GPU: LOCAL_RANK) */
int pbrhip_set_device(int device);

/* ---- scene construction: pbrlab::Scene (src/scene.h:14-111) ---- */
int pbrhip_scene_create(pbrhip_scene** out); /* Scene::Scene, scene.cc:11 */
int pbrhip_scene_destroy(pbrhip_scene*);     /* Scene::~Scene, scene.cc:12 */

/* Scene::AddTriangleMesh (scene.h:19-24) with the TriangleMesh ctor (mesh/triangle-mesh.cc:17-57) and the
 * shared Attribute buffers (mesh/attribute.h:8-12).  The reference shares the buffers by pointer
 * (raytracer.h:34); this call copies them.  normal_ids / texcoord_ids / material_ids may be NULL
 * (ids default to uint32(-1)).  vertices: xyzw * num_vertices, normals: xyzw, texcoords: uv. */
int pbrhip_scene_add_triangle_mesh(pbrhip_scene*, const float* vertices_xyzw, uint32_t num_vertices,
                                   const float* normals_xyzw, uint32_t num_normals, const float* texcoords_uv,
                                   uint32_t num_texcoords, const uint32_t* vertex_ids, const uint32_t* normal_ids,
                                   const uint32_t* texcoord_ids, const uint32_t* material_ids, uint32_t num_faces,
                                   uint32_t* mesh_id);
/* Scene::AddCubicBezierCurveMesh (scene.h:26-32, mesh/cubic-bezier-curve-mesh.cc:7-15):
 * vertices xyz+radius, indices = first control point of each cubic segment */
int pbrhip_scene_add_curve_mesh(pbrhip_scene*, const float* vertices_xyzr, uint32_t num_vertices,
                                const uint32_t* indices, const uint32_t* material_ids, uint32_t num_segments,
                                uint32_t* mesh_id);
/* Scene::AddMaterialParam (scene.h:39-44) for the two alternatives of MaterialParameter */
int pbrhip_scene_add_principled_material(pbrhip_scene*, const pbrhip_principled_param*, uint32_t* material_id);
int pbrhip_scene_add_hair_material(pbrhip_scene*, const pbrhip_hair_param*, uint32_t* material_id);
/* Scene::AddTexture (scene.h:46-51) with pbrlab::Texture (src/texture.h:13-44): float pixels, row-major, `channels`
 * (1..4) interleaved; sampled bilinearly with clamp addressing like Texture::FetchFloat3 (texture.cc:43-68,
 * image-utils.cc:99-167).  Referenced by base_color_tex_id / subsurface_color_tex_id; ids are checked at commit. */
int pbrhip_scene_add_texture(pbrhip_scene*, const float* pixels, uint32_t width, uint32_t height, uint32_t channels,
                             uint32_t* texture_id);
/* Scene::AddLightParam (scene.h:34-37) with AreaLightParameter (light-param.h:20-23) */
int pbrhip_scene_add_area_light(pbrhip_scene*, const float emission[3], uint32_t* light_id);
/* Scene::CreateLocalScene (scene.cc:157-164), AddMeshToLocalScene (scene.cc:14-62), CreateInstance (scene.cc:106-155;
 * transform = float[4][4], row-vector convention v' = v*M with the translation in the last row, NULL = identity.  As in the
 * reference the transform only reaches the raytracer (raytracer_impl.cc:61-81 hands it to Embree): rays see the transformed
 * geometry -- triangles and curve control points transformed, curve radii as they are -- while geometric / shading normals,
 * texcoords and light sampling stay in the instance's local space (scene.cc:217,237 and light-manager.h:128-136 "TODO
 * transform").  A singular or non-finite matrix is refused (PBRHIP_EINVAL). */
int pbrhip_scene_create_local_scene(pbrhip_scene*, uint32_t* local_scene_id);
int pbrhip_scene_add_mesh_to_local_scene(pbrhip_scene*, uint32_t local_scene_id, uint32_t mesh_id, uint32_t* geom_id);
int pbrhip_scene_create_instance(pbrhip_scene*, uint32_t local_scene_id, const float* transform4x4,
                                 uint32_t* instance_id);
/* Scene::AttachLightParamIdsToInstance / AttachMaterialParamIdsToInstance (scene.cc:64-94), one geometry at a
 * time; a size mismatch returns PBRHIP_ESIZE where the reference throws std::runtime_error */
int pbrhip_scene_attach_light_ids(pbrhip_scene*, uint32_t instance_id, uint32_t geom_id, const uint32_t* light_ids,
                                  uint32_t n);
int pbrhip_scene_attach_material_ids(pbrhip_scene*, uint32_t instance_id, uint32_t geom_id,
                                     const uint32_t* material_ids, uint32_t n);
/* Scene::CommitScene (scene.cc:96-104): light tables (LightManager::RegisterInstanceMesh/Commit,
 * light-manager.cc:29-184), BVH build + flatten (replaces Embree's rtcCommitScene, raytracer_impl.cc:93-197),
 * upload to HBM, scene bounds (rtcGetSceneBounds, raytracer_impl.cc:199-211) */
int pbrhip_scene_commit(pbrhip_scene*);
/* Which builder pbrhip_scene_commit uses for the acceleration structure (the reference has one: Embree's, behind
 * rtcCommitScene, raytracer_impl.cc:136-147,181-192).  HOST_SAH (default): binned SAH on the host cores, the best tree.
 * GPU_LBVH: Morton-order linear BVH built on the GPU -- commit in milliseconds for edit -> re-render loops and
 * multi-million-primitive hair, at a higher traversal cost.  Rendered images do not depend on the choice.
 * Call before pbrhip_scene_commit.  (Environment override: PBRHIP_BVH=gpu|host.) */
#define PBRHIP_BVH_HOST_SAH 0
#define PBRHIP_BVH_GPU_LBVH 1
/* GPU_LBVH_WIDE: the same tree, then collapsed on the GPU into the 4-wide quantised tree the production traversal reads (DESIGN.md
 * section 8, "The collapse, exactly"): a GPU_LBVH commit plus a few kernels, rendered by the kernels a host-built scene runs, random
 * walks' entry cuts included.  The binary tree stays (PBRHIP_WIDE=0 selects it).  A collapsed tree that cannot be kept (stack need
 * beyond the traversal stack, a record index beyond its reference, a node that cannot be quantised) is dropped with one line on stderr
 * and the scene is committed as by GPU_LBVH.  (Environment override: PBRHIP_BVH=gpu-wide.) */
#define PBRHIP_BVH_GPU_LBVH_WIDE 2
int pbrhip_scene_set_bvh_builder(pbrhip_scene*, int builder);
/* The 4-wide quantised tree of a committed scene: its nodes (0: none -- PBRHIP_WIDE=0 at commit, builder GPU_LBVH, or a dropped tree),
 * the exact traversal-stack need of a near-first traversal, and whether it was collapsed on the GPU.  Any pointer may be NULL. */
int pbrhip_scene_wide_info(const pbrhip_scene*, uint64_t* wide_nodes, uint32_t* stack_need, int* built_on_gpu);
/* Scene::FetchSceneAABB (scene.cc:251-259) */
int pbrhip_scene_aabb(const pbrhip_scene*, float bmin[3], float bmax[3]);
/* Scene::FetchMeshMaterialParameters + EditQueue edits between renders (pc/pc-common.cc:57-84): replace one
 * material's parameters in place on a committed scene */
int pbrhip_scene_update_principled_material(pbrhip_scene*, uint32_t material_id, const pbrhip_principled_param*);
int pbrhip_scene_update_hair_material(pbrhip_scene*, uint32_t material_id, const pbrhip_hair_param*);
/* Geometry edits between renders ("The refit, exactly").  The update calls replace VALUES of the host model: a triangle
 * mesh's vertices (and its normals; NULL: kept), a curve mesh's control points xyzr, an instance's transform (NULL: identity).  Indices,
 * texcoords, materials and light attachments stay: the topology is fixed.  Counts must equal the mesh's own (else PBRHIP_ESIZE); a
 * non-finite value, a mesh of the other kind, an id out of range or a matrix pbrhip_scene_create_instance would refuse: PBRHIP_EINVAL,
 * and nothing changes.  Before the first commit they only edit the model.  On a committed scene every instance that shows the mesh (or
 * the one instance) becomes dirty and the scene STALE: until pbrhip_scene_refit (or another pbrhip_scene_commit, which rebuilds from the
 * model) every entry point that reads the device scene -- pbrhip_render*, pbrhip_render_features*, pbrhip_trace_*, pbrhip_camera_rays,
 * pbrhip_scene_aabb, pbrhip_scene_replicate, pbrhip_comm_gather_layer -- returns PBRHIP_ESTATE.
 * pbrhip_scene_refit brings the committed scene up to date ON THE DEVICE: the trees keep the topology their builder gave them and every
 * stored box, leaf record, slot, ShadeRec, light table, the scene's bounds and the random walks' entries are recomputed, so that every
 * observable (hits, pbrhip_scene_aabb, frames, feature buffers) equals, bit for bit, that of a fresh scene built from the edited model
 * and committed with the same builder.  Only the tree's QUALITY is the old pose's: after large motions a commit traces faster.
 * Uncommitted scene: PBRHIP_ESTATE; nothing pending: PBRHIP_OK, nothing happens.  A Q node that cannot be quantised (it cannot arise
 * from finite vertices): PBRHIP_EHIP, the scene stays stale.  A replica made by pbrhip_scene_replicate holds no geometry: the update
 * calls and pbrhip_scene_refit return PBRHIP_ESTATE on it -- refit the source scene and replicate it again. */
int pbrhip_scene_update_triangle_mesh(pbrhip_scene*, uint32_t mesh_id, const float* vertices_xyzw, uint32_t num_vertices,
                                      const float* normals_xyzw, uint32_t num_normals);
int pbrhip_scene_update_curve_mesh(pbrhip_scene*, uint32_t mesh_id, const float* vertices_xyzr, uint32_t num_vertices);
int pbrhip_scene_update_instance_transform(pbrhip_scene*, uint32_t instance_id, const float* transform4x4);
int pbrhip_scene_refit(pbrhip_scene*);
/* The same mesh edits from DEVICE memory, for a simulation that holds its vertices on the scene's GPU (a torch tensor's data_ptr()):
 * d_vertices_xyzw / d_normals_xyzw / d_vertices_xyzr are device pointers of the scene's device (anything else, host memory included:
 * PBRHIP_EINVAL), 16-byte aligned; `stream` is the caller's hipStream_t (NULL: the null stream).  The library reads the arrays only
 * after the work already enqueued on that stream (an event and a stream wait, no device-wide synchronise), checks them for non-finite
 * values on the device, and holds its own copy when the call returns: the caller may overwrite the buffer.  Counts, refusals and their
 * codes are the host calls'; after a refusal nothing has changed.  The host model receives the values inside the call (a download), so
 * pbrhip_scene_commit, the light tables and the host calls keep working.  Before the first commit the call only edits the model.
 * The first successful call on a committed scene switches the scene to DEVICE GEOMETRY MODE until the next commit: every mesh's
 * position, normal and index arrays are uploaded once, the host update calls refresh that copy as well, and pbrhip_scene_refit
 * re-derives the dirty instances' slots, ShadeRecs and bounds on the device from it ("Staging on the device")
 * instead of staging them on the host -- with the same functions, so the refitted scene is the same, bit for bit.  (One freedom: a
 * scene bound taken over both +0 and -0 is -0 as a minimum and +0 as a maximum; the host's chain of fminf gives either.)  A scene that
 * never makes these calls allocates nothing for them. */
int pbrhip_scene_update_triangle_mesh_device(pbrhip_scene*, uint32_t mesh_id, const void* d_vertices_xyzw, uint32_t num_vertices,
                                             const void* d_normals_xyzw, uint32_t num_normals, void* stream);
int pbrhip_scene_update_curve_mesh_device(pbrhip_scene*, uint32_t mesh_id, const void* d_vertices_xyzr, uint32_t num_vertices, void* stream);
/* A test hook: the committed scene's slots (64 bytes each, leaf order) and ShadeRecs (128 bytes each) as the device holds them, so that
 * a stale word no ray happens to see can still be found.  num_slots receives the count; with both output pointers NULL nothing else
 * happens.  Uncommitted or stale scene: PBRHIP_ESTATE. */
int pbrhip_scene_read_slots(pbrhip_scene*, void* slots_out, void* shade_out, uint32_t* num_slots);
/* A lat-long environment light: rgb = width x height x 3 floats, row 0 = the top (+y up; a ray along -z sees the
 * middle of the map), nearest-sampled, times `scale`.  world_to_env: a 3x3 rotation, row-major, applied to world directions before
 * the lookup (NULL: identity).  A ray that leaves the scene collects it (with MIS), and NEE samples it by luminance x solid angle.
 * rgb == NULL removes the environment; an all-black map is no environment.  Valid before or after pbrhip_scene_commit: takes
 * effect at the next render.  A negative, NaN or infinite texel or scale, a zero size or a matrix that is no rotation:
 * PBRHIP_EINVAL.  The map is copied. */
int pbrhip_scene_set_environment(pbrhip_scene*, const float* rgb, uint32_t width, uint32_t height, float scale,
                                 const float world_to_env[9]);
/* A look-at camera in place of the reference's, which is fitted to the scene's box and looks down -z.  f = normalize(lookat
 * - eye), r = normalize(f x up), u = r x f; pixel (x, y) (row 0 = the top) with jitter (jx, jy) -- the sample's first two draws -- sees
 * along f + sx r + sy u, sx = (2 (x + jx) / W - 1) tan(vfov / 2) W / H, sy = (1 - 2 (y + jy) / H) tan(vfov / 2); vfov in degrees.
 * lens_radius 0: a pinhole at eye.  lens_radius > 0: a thin lens -- two more draws u1, u2 pick the origin eye + rho (cos phi r + sin phi u),
 * rho = lens_radius sqrt(u1), phi = 2 pi u2, and the ray passes through the pixel's point at distance focus_distance along f
 * (0: |lookat - eye|), which is in focus.  eye == NULL restores the reference's camera.  Valid before or after pbrhip_scene_commit: takes
 * effect at the next render (a PBRHIP_RENDER_NO_CLEAR render after a change mixes the two views).  A non-finite value, eye == lookat, up
 * (nearly) parallel to lookat - eye, vfov outside (0, 180), a negative lens_radius or focus_distance: PBRHIP_EINVAL, and the camera
 * stays as it was.  pbrhip_scene_replicate carries it over. */
int pbrhip_scene_set_camera(pbrhip_scene*, const float eye[3], const float lookat[3], const float up[3], float vfov_degrees,
                            float lens_radius, float focus_distance);
/* BVH facts for reports: node count, leaf slots, depth, device bytes */
int pbrhip_scene_info(const pbrhip_scene*, uint64_t* num_nodes, uint64_t* num_slots, uint32_t* depth,
                      uint64_t* device_bytes);

/* ---- the hot path ---- */
/* pbrlab::Render (src/render.h:14-17, render.cc:192-241).  Blocking.  rgba: width*height*4 floats (sum of
 * radiance, A = sample count), count: width*height (RenderLayer, render-layer.h:11-26).
 *
 * cancel: NULL or the address of a byte another thread may set non-zero while the call runs -- the object
 * representation of the reference's `const std::atomic_bool& cancel_render_flag` (a lock-free byte).  It is read live
 * at every host round trip of the render loop (once per wavefront iteration of a path group, i.e. every few
 * milliseconds at most; the reference polls before every tile job, render.cc:217).  A cancelled call drains what is in
 * flight, drops the passes that are not complete and returns PBRHIP_OK with a consistent layer: every pixel of this rank
 * holds exactly *finish_pass passes.
 * finish_pass: NULL or a size_t (the reference's std::atomic_size_t, render.cc:224-231) that is stored to (atomically,
 * monotone) while the call runs, each time a further group of passes is complete for every pixel.
 * Per-sample RNG: RNG((pass << 32) + y*width + x, seed_seq). */
int pbrhip_render(pbrhip_scene*, const pbrhip_render_desc*, const volatile unsigned char* cancel, float* rgba,
                  uint32_t* count, size_t* finish_pass, pbrhip_render_stats* stats);
/* Same, writing into DEVICE buffers owned by the caller (e.g. a torch tensor that is then exchanged over RCCL):
 * d_rgba / d_count are device pointers on the scene's device; nothing is copied to the host. */
int pbrhip_render_device(pbrhip_scene*, const pbrhip_render_desc*, const volatile unsigned char* cancel, float* d_rgba,
                         uint32_t* d_count, size_t* finish_pass, pbrhip_render_stats* stats);

/* ---- first-hit feature buffers and the denoiser ---- */
/* What the camera saw first, summed per pixel over the passes [first_pass, first_pass + num_sample) of the frame pbrhip_render makes
 * from the same descriptor (the same camera rays: pbrhip_camera_rays; the same closest hits: pbrhip_trace_closest):
 *   albedo_hits   W*H*4: sum of the albedo rgb over the samples that hit | number of samples that hit
 *   normal_depth  W*H*4: sum of the shading normal (Surface::n_s, turned towards the viewer; a curve's tangent as it is) |
 *                        sum of the hit distance t, over the same samples
 *   count         W*H:   samples taken (hits + misses), like the RenderLayer's
 * Any of the three may be NULL (not wanted).  albedo: a principled material's base_color (its map at the hit's texcoords when it has
 * one), a hair material's base_color, or for melanin the colour with the material's sigma_a; no material: black.  A miss adds
 * nothing but 1 to count.  The sums are float32 in ascending pass order per pixel: bit-identical under any max_paths_in_flight,
 * shard_block or tree builder.  tile_rank / tile_world / shard_block select pixels as in pbrhip_render; PBRHIP_RENDER_NO_CLEAR
 * accumulates on top of the caller's buffers (which continues the sums: passes [0, 4) then [4, 8) == [0, 8)); other flags,
 * num_streams and tail_paths are ignored.  Errors as pbrhip_render's; zero samples: PBRHIP_EINVAL. */
int pbrhip_render_features(pbrhip_scene*, const pbrhip_render_desc*, float* albedo_hits, float* normal_depth, uint32_t* count);
/* Same, into DEVICE buffers on the scene's device. */
int pbrhip_render_features_device(pbrhip_scene*, const pbrhip_render_desc*, float* d_albedo_hits, float* d_normal_depth,
                                  uint32_t* d_count);

/* Edge-avoiding A-trous filter (Dammertz et al. 2010) of a RenderLayer (rgba sums + count) guided by the feature buffers above; needs
 * no scene.  out_rgba: W*H*4, the denoised MEAN colour | 1 ((0, 0, 0, 0) where count == 0).  Per pixel p: c = rgb / count; albedo
 * a = (albedo_hits.rgb + misses) / feature_count (a miss counts as white; 1 without features or with PBRHIP_DENOISE_NO_ALBEDO);
 * e(0) = c / max(a, 1e-3); N = normalised normal sum, z = depth sum / hits (a pixel without hits is background).  Iteration
 * i = 0 .. iterations - 1 with step s = 2^i: e(i+1)_p = sum_q h w e(i)_q / sum_q h w over the 25 taps q = p + s (dx, dy), |dx|, |dy| <= 2,
 * inside the image and with count != 0; h = B3 spline [1 4 6 4 1] / 16 in x and y; w(p, p) = 1, else w = w_n w_z w_c:
 *   w_n = max(0, N_p . N_q)^(2^normal_squarings) (1 between two background pixels, 0 between a background pixel and a surface)
 *   w_z = exp(-|z_p - z_q| / (sigma_depth z_p |q - p|))     (|q - p| in pixels; 1 between background pixels or when sigma_depth <= 0)
 *   w_c = exp(-|e_p - e_q|^2 / (sigma_color 2^-i)^2)         (1 when sigma_color <= 0)
 * out.rgb = e(iterations) a.  iterations: 1 .. 8, 0 = PBRHIP_DENOISE_ITERATIONS.  A non-positive sigma switches its weight off (it is
 * never read as "default": pass the macros).  albedo_hits, normal_depth and feature_count may all three be NULL: a colour-guided
 * A-trous.  PBRHIP_EINVAL: a NaN sigma, iterations > 8, normal_squarings > 16, a zero size, a NULL rgba / count / out_rgba, some but
 * not all of the three feature buffers.  The sigmas below were chosen on the Cornell
 * variants at 4-16 spp, 256 x 256, by relative MSE against 4096 spp: the 8-spp GGX frame goes from 0.0326 to 0.0189 (what 14 spp reach),
 * its wall interiors from 0.0331 to 0.0028 (95 spp); the optimum sigma_color falls with the noise: 1 at 4 spp, 0.25 at 16.
 * With the colour weight off an emitter of black albedo bleeds into its neighbours (its e is c / 1e-3): keep it on for lit scenes. */
#define PBRHIP_DENOISE_NO_ALBEDO 1u /* filter the colour itself, not colour / albedo */
#define PBRHIP_DENOISE_ITERATIONS 5
#define PBRHIP_DENOISE_NORMAL_SQUARINGS 7
#define PBRHIP_DENOISE_SIGMA_COLOR 0.5f
#define PBRHIP_DENOISE_SIGMA_DEPTH 0.2f
int pbrhip_denoise(int device, uint32_t width, uint32_t height, const float* rgba, const uint32_t* count, const float* albedo_hits,
                   const float* normal_depth, const uint32_t* feature_count, uint32_t iterations, float sigma_color, float sigma_depth,
                   uint32_t normal_squarings, uint32_t flags, float* out_rgba);
/* Same with DEVICE pointers on `device`. */
int pbrhip_denoise_device(int device, uint32_t width, uint32_t height, const float* d_rgba, const uint32_t* d_count,
                          const float* d_albedo_hits, const float* d_normal_depth, const uint32_t* d_feature_count, uint32_t iterations,
                          float sigma_color, float sigma_depth, uint32_t normal_squarings, uint32_t flags, float* d_out_rgba);

/* ---- adaptive sampling ----
 * pbrhip_render with a sample count per 8x8 TILE: tiles whose error estimate has fallen to `threshold` stop, the rest render on, up to
 * desc->num_sample passes (the maximum level).  The contract: pixel p of the layer holds, bit for bit, what pbrhip_render with
 * num_sample = count[p] (same descriptor otherwise) holds at p -- a pixel's value is a function of (pixel, pass) and its float sums run in
 * ascending pass order, however the passes were grouped.  Which count a pixel gets is defined exactly:
 *   tiles   8x8 pixels aligned to the image origin, clipped at the right and bottom edges; id = ty * ceil(W / 8) + tx.  shard_block must be
 *           a multiple of 8 (0 = 64), so that every tile belongs to one rank.
 *   levels  n_0 = first_level (0 = PBRHIP_ADAPTIVE_FIRST_LEVEL), n_k = min(2 n_(k-1), num_sample).  Round 0 renders the passes [first_pass,
 *           first_pass + n_0) of every pixel of the rank, round k >= 1 the passes [first_pass + n_(k-1), first_pass + n_k) of the pixels of
 *           the tiles still active.  A decision follows every round k >= 1 (so every pixel holds at least min(2 first_level, num_sample)
 *           passes); a stopped tile never restarts.  first_level >= num_sample: one plain round of num_sample, no decision.
 *   error   with A the layer at level n_(k-1) and I the layer at level n_k, per pixel in float32, every operation rounded once:
 *           a = A.rgb / (float)n_(k-1), b = (I.rgb - A.rgb) / (float)(n_k - n_(k-1)), m = I.rgb / (float)n_k,
 *           d = |a.r - b.r| + |a.g - b.g| + |a.b - b.b|, s = m.r + m.g + m.b (both left to right), e = d / sqrtf(s + 1e-3f)
 *           (the 1e-3f keeps black pixels finite: a design constant).  E = the float64 sum of the tile's e, lane (y & 7) * 8 + (x & 7),
 *           absent lanes of a clipped tile 0, as a butterfly over the xor distances 1, 2, 4, 8, 16, 32, divided by the tile's pixel count.
 *   stop    when E <= (double)threshold; a NaN E compares false and the tile stays active.
 * tile_error: ceil(W / 8) * ceil(H / 8) floats, a tile's last (float)E (a NaN as 0x7FC00000); 0 for tiles of other ranks and for tiles no
 * decision reached.  *finish_pass is stored after every round with the level every pixel of the rank holds; *samples = the sum of count
 * over the rank's pixels; *rounds = the rounds rendered.  tile_error, finish_pass, samples and rounds may be NULL.
 * max_paths_in_flight, num_streams, tail_paths, seed_seq, tile_rank / tile_world / shard_block act as in pbrhip_render and do not change
 * the result; PBRHIP_RENDER_NO_CLEAR is refused (an adaptive layer cannot be resumed), other flags are ignored.
 * PBRHIP_EINVAL: a NULL scene, descriptor or layer, PBRHIP_RENDER_NO_CLEAR, a negative or NaN threshold, shard_block % 8 != 0,
 * num_sample == 0; an uncommitted or stale scene: PBRHIP_ESTATE.  cancel: the round in flight ends as pbrhip_render's does (the active
 * pixels hold n_(k-1) + the passes that were complete), no decision follows, the call returns PBRHIP_OK and the contract above holds.
 * BIAS: stopping on an estimate made from the samples themselves is biased, as in every such scheme (a tile that looks converged by
 * chance stops early and keeps its luck).  The guards are the two-level minimum and the tile mean: 64 pixels decide together.
 * Not provided: dilation of the active set into neighbouring tiles, lists finer than a tile, a pbrhip_render_multi twin (render the
 * shards with tile_rank / tile_world and add them), resuming an adaptive layer.
 * PBRHIP_ADAPTIVE_THRESHOLD: see profiles/README.md ("Adaptive sampling") for the sweep behind the value. */
#define PBRHIP_ADAPTIVE_FIRST_LEVEL 8u
#define PBRHIP_ADAPTIVE_THRESHOLD 0.07f
int pbrhip_render_adaptive(pbrhip_scene*, const pbrhip_render_desc*, float threshold, uint32_t first_level,
                           const volatile unsigned char* cancel, float* rgba, uint32_t* count, float* tile_error, size_t* finish_pass,
                           uint64_t* samples, uint32_t* rounds);
/* Same, into DEVICE buffers on the scene's device (d_tile_error may be NULL). */
int pbrhip_render_adaptive_device(pbrhip_scene*, const pbrhip_render_desc*, float threshold, uint32_t first_level,
                                  const volatile unsigned char* cancel, float* d_rgba, uint32_t* d_count, float* d_tile_error,
                                  size_t* finish_pass, uint64_t* samples, uint32_t* rounds);
/* One decision step without a scene (host pointers): a test hook.  rgba = I at level n_now, snapshot_inout = A at level n_prev (on
 * return: I for the pixels of the tiles of tiles_in), tiles_in = num_tiles_in distinct tile ids.  tiles_out / pixels_out (room for
 * num_tiles_in ids / width * height pixels) receive the tiles that stay active, in the order they had, and their pixels, tile after
 * tile and row-major inside a tile; tile_error_inout (ceil(W / 8) * ceil(H / 8)) receives the E of the tiles of tiles_in. */
int pbrhip_adaptive_step(int device, uint32_t width, uint32_t height, const float* rgba, float* snapshot_inout, uint32_t n_prev,
                         uint32_t n_now, float threshold, const uint32_t* tiles_in, uint32_t num_tiles_in, uint32_t* tiles_out,
                         uint32_t* num_tiles_out, uint32_t* pixels_out, uint32_t* num_pixels_out, float* tile_error_inout);

/* ---- rendering along caller-supplied rays ----
 * pbrhip_render with the first ray of every sample read from a buffer instead of computed by the scene's camera: a sensor model of the
 * caller's own (a distorted lens, a lidar pattern, a stereo pair, a ring of probes), or one of the projections below.
 *   rays        desc->width x desc->height is the shape of the ray grid; the ray of (pixel y * width + x, pass) is
 *               rays[(ray_passes == 1 ? 0 : pass - desc->first_pass) * width * height + y * width + x].  ray_passes: 1 (one ray per pixel,
 *               reused by every pass) or desc->num_sample; anything else is PBRHIP_EINVAL.
 *   a ray       is traced as given: org, dir, and the interval [tmin, tmax] for the first segment.  dir must be of unit length; it is
 *               NOT renormalised (that would change its bits).
 *   generator   the path of (pixel, pass) draws from the generator every sample of this renderer owns, seeded with (pass << 32) + pixel
 *               and desc->seed_seq, advanced by camera_draws draws (0 .. 16) first: a caller who builds its rays from the first draws of
 *               that generator passes how many it took and gets path draws that do not repeat them.  With the rays of pbrhip_camera_rays
 *               for every (pixel, pass) and camera_draws = 2 (the reference's camera, a pinhole) or 4 (a thin lens) the frame equals
 *               pbrhip_render's bit for bit; so it does under any max_paths_in_flight, num_streams, tail_paths, tile_rank / tile_world /
 *               shard_block, first_pass with PBRHIP_RENDER_NO_CLEAR (with per-pass rays the call's buffer starts at ITS first pass) and
 *               tree builder, which all act as in pbrhip_render.
 *   inactive    a ray with a NaN among its eight numbers, an infinite origin or direction component, a zero direction, tmin < 0 or
 *               !(tmax >= tmin) is inactive: its sample adds exactly (0, 0, 0, 1) to rgba and 1 to count -- no fault, no environment.
 * pbrhip_render_rays takes host rays; pbrhip_render_rays_device takes rays in device memory of the scene's device and `stream`, the
 * stream they are produced on: they are read only after the work already enqueued there (pbrhip_scene_update_triangle_mesh_device's
 * rule; the call itself is synchronous like pbrhip_render_device).  cancel, finish_pass, stats: as pbrhip_render's.
 * PBRHIP_EINVAL ("NULL" in pbrhip_last_error) for a NULL scene, descriptor, rays or layer; PBRHIP_EINVAL for a bad ray_passes or
 * camera_draws > 16, before any device work; then pbrhip_render's errors.
 * Not provided: a ray source for pbrhip_render_multi, pbrhip_render_adaptive and the RCCL gather (render the shards with tile_rank /
 * tile_world, which work here, and add them). */
int pbrhip_render_rays(pbrhip_scene*, const pbrhip_render_desc*, const pbrhip_ray* rays, uint32_t ray_passes, uint32_t camera_draws,
                       const volatile unsigned char* cancel, float* rgba, uint32_t* count, size_t* finish_pass, pbrhip_render_stats*);
int pbrhip_render_rays_device(pbrhip_scene*, const pbrhip_render_desc*, const void* d_rays, uint32_t ray_passes, uint32_t camera_draws,
                              void* stream, const volatile unsigned char* cancel, float* d_rgba, uint32_t* d_count, size_t* finish_pass,
                              pbrhip_render_stats*);
/* pbrhip_render_features_device over the same rays (layout, ray_passes, stream, inactive rays -- a miss -- as above): with the rays of
 * pbrhip_camera_rays the buffers equal pbrhip_render_features' bit for bit.  The traversal starts from each ray's tmin and tmax. */
int pbrhip_render_features_rays_device(pbrhip_scene*, const pbrhip_render_desc*, const void* d_rays, uint32_t ray_passes, void* stream,
                                       float* d_albedo_hits, float* d_normal_depth, uint32_t* d_count);
/* The rays of three projections, written on the device into d_rays (num_pass x width x height pbrhip_ray, pass-major: the layout
 * pbrhip_render_rays_device takes with ray_passes = num_pass, first_pass = desc->first_pass, camera_draws = 2), asynchronously on `stream`.
 * The frame is the scene's pbrhip_scene_set_camera one (eye; f towards lookat, r = f x up, u = r x f, normalised); PBRHIP_ESTATE when the
 * scene has none.  With jx, jy the first two draws of the sample's generator, sx = 2 (x + jx) / W - 1, sy = 1 - 2 (y + jy) / H and
 * aspect = W / H, in float32:
 *   LATLONG  phi = 2 pi (x + jx) / W - pi, theta = pi (y + jy) / H, dir = sin theta sin phi r + cos theta u + sin theta cos phi f: a 360 degree
 *            panorama, the inverse of the environment light's texel mapping with the image centre along f.  param is ignored.
 *   FISHEYE  equidistant: rho = sqrt((sx aspect)^2 + sy^2), angle = rho fov / 2, dir = sin(angle) (sx aspect r + sy u) / rho + cos(angle) f;
 *            rho = 0: f; rho > 1: an inactive ray (the corners of the frame are black).  param: fov in degrees, up to 360; 0 = the
 *            camera's vertical field of view.
 *   ORTHO    org = eye + sx aspect param r + sy param u, dir = f; param: half the height of the view in world units, > 0.
 * tmin = 0, tmax as the cameras'.  The scene need not be committed. */
enum { PBRHIP_PROJECTION_LATLONG = 0, PBRHIP_PROJECTION_FISHEYE = 1, PBRHIP_PROJECTION_ORTHO = 2 };
int pbrhip_projection_rays_device(pbrhip_scene*, uint32_t projection, float param, uint32_t width, uint32_t height, uint32_t first_pass,
                                  uint32_t num_pass, uint64_t seed_seq, void* d_rays, void* stream);

/* ---- motion vectors and temporal accumulation across refits ----
 * For a sequence rendered at a few samples per pixel per frame: where the surface point seen in each pixel was one frame ago, and an
 * accumulation that re-uses the previous frames' samples there and rejects history where the point was hidden.  Per frame:
 *   pbrhip_scene_snapshot_pose -> pbrhip_scene_update_* / pbrhip_scene_set_camera -> pbrhip_scene_refit -> pbrhip_render ->
 *   pbrhip_render_motion -> pbrhip_temporal_accumulate (-> pbrhip_denoise of the accumulated mean).
 *
 * pbrhip_scene_snapshot_pose keeps a device-to-device copy of what defines the pose of a committed scene: its slots (64 bytes each,
 * world space: a triangle's corners, a curve piece's two end points) and the camera state in effect -- pbrhip_scene_set_camera's
 * arguments, or without a user camera the scene's bounds, which the reference's camera is derived from (it moves when they do).  The copy
 * is ordered on the scene's stream.  A second call replaces the first.  The snapshot survives pbrhip_scene_update_*, pbrhip_scene_refit
 * (host path and device geometry mode), material updates, pbrhip_scene_set_camera and pbrhip_scene_set_environment; pbrhip_scene_commit
 * drops it (slot order changes); pbrhip_scene_replicate does not carry it.  An uncommitted or stale scene: PBRHIP_ESTATE.  A scene that
 * never calls it allocates nothing. */
int pbrhip_scene_snapshot_pose(pbrhip_scene*);
/* Per pixel (x, y) of the rank's pixels (tile_rank / tile_world / shard_block select them as in pbrhip_render_features; the other
 * pixels of the buffers are zeroed): the pixel-CENTRE ray of the scene's current camera -- jitter jx = jy = 0.5, the lens point at the lens
 * centre, so a pinhole even when a thin lens is set; the cameras' own arithmetic -- and its closest hit.  No generator is involved:
 * num_sample, first_pass, seed_seq, flags, max_paths_in_flight, num_streams and tail_paths are ignored.  Each output may be NULL.
 *   ident   W*H*4 uint32: slot (the hit's index into pbrhip_scene_read_slots' arrays), then the bits of u, v, t: what
 *           pbrhip_trace_closest reports for that ray, bit for bit; a miss: (PBRHIP_NONE, 0, 0, 0).  Also a picking buffer.
 *   guide   W*H*4 float: the shading normal (Surface::n_s) turned towards the viewer -- a curve's tangent as it is -- | t; a miss: zeros.
 *   motion  W*H*4 float: (mx, my, z_prev, valid).  X_prev = the hit's point on the snapshot's pose: (1 - u - v) v0 + u v1 + v v2 of the
 *           snapshot's slot for a triangle; for a curve the point a + (4 u - sub) (b - a) on the axis of the snapshot's piece (u is the
 *           cubic's parameter, the piece covers [sub / 4, (sub + 1) / 4]: the centre line the traversal tests; the ribbon's width is
 *           ignored).  (px, py) = the continuous pixel coordinates at which the snapshot's pinhole camera -- the one pbrhip_render would
 *           have derived from the snapshot's state for desc->width x desc->height -- sees X_prev; mx = px - (x + 0.5),
 *           my = py - (y + 0.5), z_prev = |X_prev - eye_prev|.  valid = 1 (a triangle) or 2 (a curve: the accumulation's normal test
 *           takes |N . N| for it, a tangent has no facing -- guide has no component to spare for that mark, its .w is t bit for bit)
 *           when the ray hit and X_prev lies in front of the snapshot's camera, else the whole value is (0, 0, 0, 0).  A point outside
 *           the frame keeps its valid: the accumulation decides.
 * The results do not depend on the tree builder, shard_block or PBRHIP_WIDE.  No snapshot: PBRHIP_ESTATE; the other errors are
 * pbrhip_render_features'.  Not provided: caller-supplied ray lists and the lat-long / fisheye / ortho projections, motion through the
 * thin lens, motion of the environment background. */
int pbrhip_render_motion(pbrhip_scene*, const pbrhip_render_desc*, float* motion, float* guide, uint32_t* ident);
/* Same, into DEVICE buffers on the scene's device. */
int pbrhip_render_motion_device(pbrhip_scene*, const pbrhip_render_desc*, float* d_motion, float* d_guide, uint32_t* d_ident);
/* The reprojecting accumulation; needs no scene.  rgba / count: the current frame's RenderLayer; motion / guide: the current frame's
 * pbrhip_render_motion buffers; hist_rgba: W*H*4, the accumulated mean | history length (a previous call's out_rgba); hist_guide: the
 * guide of the frame hist_rgba was made for; both NULL: no history.  out_rgba: W*H*4, the new mean | the new history length (it must not
 * be hist_rgba; the guide to hand in with the next frame is this frame's guide).  Per pixel (x, y), float32, every operation rounded
 * once: c = rgb / count; count == 0: out = (0, 0, 0, 0); valid == 0 or no history: out = (c, 1).  Otherwise q = (x + mx, y + my),
 * x0 = floor(q.x), y0 = floor(q.y), f = q - (x0, y0); the taps (x0 + i, y0 + j), i, j in {0, 1}, in the order (0, 0) (1, 0) (0, 1) (1, 1),
 * with the weights w = (i ? f.x : 1 - f.x) (j ? f.y : 1 - f.y).  A tap is accepted when it is inside the image, its history length is > 0,
 * hist_guide.w > 0, |hist_guide.w - z_prev| <= sigma_depth z_prev and N_hist . N_now >= normal_cos_min (|N_hist . N_now| when valid == 2).
 * S = the sum of the accepted weights; S == 0: out = (c, 1).  Otherwise h = sum(w hist.rgb) / S, n = sum(w hist.len) / S,
 * len = min(n + 1, max_history), a = max(1 / len, alpha_min), out = (h + a (c - h), len).
 * PBRHIP_EINVAL, before any device work: a NULL rgba, count, motion, guide or out_rgba, one of hist_rgba / hist_guide without the other,
 * out_rgba == hist_rgba, a NaN parameter, max_history outside [1, 2^24], a zero size.  The parameters are never read as "default": pass
 * the macros (profiles/README.md "Temporal accumulation" has the sweep behind them).
 * Variance-guided filtering and an identity test of the history: the block below (pbrhip_svgf_accumulate, pbrhip_svgf_filter).
 * Not provided: reprojection of the background by direction, a multi-GPU twin. */
#define PBRHIP_TEMPORAL_ALPHA_MIN 0.2f
#define PBRHIP_TEMPORAL_SIGMA_DEPTH 0.05f
#define PBRHIP_TEMPORAL_NORMAL_COS_MIN 0.9f
#define PBRHIP_TEMPORAL_MAX_HISTORY 32u
int pbrhip_temporal_accumulate(int device, uint32_t width, uint32_t height, const float* rgba, const uint32_t* count, const float* motion,
                               const float* guide, const float* hist_rgba, const float* hist_guide, float alpha_min, float sigma_depth,
                               float normal_cos_min, uint32_t max_history, float* out_rgba);
/* Same with DEVICE pointers on `device`. */
int pbrhip_temporal_accumulate_device(int device, uint32_t width, uint32_t height, const float* d_rgba, const uint32_t* d_count,
                                      const float* d_motion, const float* d_guide, const float* d_hist_rgba, const float* d_hist_guide,
                                      float alpha_min, float sigma_depth, float normal_cos_min, uint32_t max_history, float* d_out_rgba);

/* ---- variance-guided filtering and identity-tested history (SVGF, Schied et al. 2017) ----
 * A second pipeline beside pbrhip_temporal_accumulate -> pbrhip_denoise, for the same sequences:
 *   pbrhip_render -> pbrhip_render_features -> pbrhip_render_motion -> pbrhip_scene_object_ids -> pbrhip_svgf_accumulate -> pbrhip_svgf_filter.
 * The accumulation also rejects history that belongs to another object and carries a per-pixel variance of what is filtered; the filter's
 * luminance weight is scaled by that variance, so a pixel with a long history is filtered narrowly and a disoccluded one widely.
 * Notation: u = 2^-24; "live" = history length > 0; lum(e) = (0.2126f e.r + 0.7152f e.g) + 0.0722f e.b.  All arithmetic is float32, every
 * operation rounded once, in the order written here; exp is the library's; square root and division are correctly rounded.
 *
 * Object ids.  ident: pbrhip_render_motion's W*H*4 buffer.  ids[p] = word 24 + what of the ShadeRec (pbrhip_scene_read_slots) of slot
 * ident[4 p]; PBRHIP_NONE for a miss and for any slot >= the scene's slot count (the kernel checks: the buffer is the caller's).  One
 * gather, a lane per pixel.  The three words do not depend on the tree builder (the slot order does).  The buffer doubles as an object
 * matte.  The device variant is ordered behind the caller's `stream` as pbrhip_render_rays_device is, and returns when the ids are
 * written.  PBRHIP_ESTATE: an uncommitted or stale scene.  PBRHIP_EINVAL: a NULL scene, a NULL buffer with num_pixels > 0, what > 2. */
#define PBRHIP_ID_PRIMITIVE 0u /* ShadeRec word 24: the canonical primitive id (gid) */
#define PBRHIP_ID_INSTANCE 1u  /* word 25 */
#define PBRHIP_ID_GEOM 2u      /* word 26 */
int pbrhip_scene_object_ids(pbrhip_scene*, const uint32_t* ident, size_t num_pixels, uint32_t what, uint32_t* ids);
int pbrhip_scene_object_ids_device(pbrhip_scene*, const void* d_ident, size_t num_pixels, uint32_t what, void* d_ids, void* stream);

/* The accumulation; needs no scene.  rgba / count, motion / guide: as pbrhip_temporal_accumulate's.  albedo_hits + feature_count
 * (pbrhip_render_features; both or neither): the albedo a = (albedo_hits.rgb + misses) / feature_count with misses = feature_count -
 * albedo_hits.w, exactly pbrhip_denoise's (a miss counts as white; 1 where feature_count == 0 or without the buffers).  ids: this frame's
 * object ids (W*H) or NULL.  History, all three or none: hist_illum W*H*4 (e.rgb | history length: a previous call's out_illum, or a
 * filter's out_feedback), hist_var W*H (that call's out_var), hist_guide W*H*4 (that frame's guide); hist_ids W*H (that frame's ids) is
 * given exactly when ids is given and the history is present.  Outputs: out_illum W*H*4 and out_var W*H; neither may be a history buffer.
 * Per pixel p: count == 0: out_illum = (0, 0, 0, 0), out_var = 0.  Otherwise c = rgb / count, e = c / max(a, 1e-3) per channel,
 * l = lum(e).  The taps, their weights and their acceptance are pbrhip_temporal_accumulate's, in its order and with its comparisons,
 * hist_illum.w in the place of the history length; with ids one more condition: hist_ids[q] == ids[p].  valid == 0, no history, or
 * S == 0: out_illum = (e, 1), out_var = 0.  Otherwise with the accepted taps' w: h = sum(w hist_illum.rgb) / S, n = sum(w hist_illum.w) / S,
 * v = sum(w hist_var) / S (each sum in tap order), len = min(n + 1, max_history), al = max(1 / len, alpha_min), d = l - lum(h),
 *   out_illum = (h + al (e - h), len),   out_var = (1 - al) (v + (al d) d).
 * Without ids and albedo out_illum is pbrhip_temporal_accumulate's out_rgba bit for bit.  The variance is the exponentially weighted
 * central form: it subtracts no large equals (mu2 - mu1^2 cancels where the variance is small against the mean, which is where the filter
 * should be wide), it is never negative, with alpha_min = 0 it is the population variance of the pixel's l so far (Welford), and the
 * mean it refers to is lum of the accumulated illumination: no moment image is carried.
 * PBRHIP_EINVAL, before any device work: pbrhip_temporal_accumulate's refusals (out_var among the outputs), alpha_min outside [0, 1],
 * one of albedo_hits / feature_count without the other, a history of one or two of its three buffers, hist_ids against the rule above,
 * an output that is a history buffer or the other output.  The parameters are never read as "default": pass the macros. */
#define PBRHIP_SVGF_ALPHA_MIN 0.2f
int pbrhip_svgf_accumulate(int device, uint32_t width, uint32_t height, const float* rgba, const uint32_t* count, const float* albedo_hits,
                           const uint32_t* feature_count, const float* motion, const float* guide, const uint32_t* ids,
                           const float* hist_illum, const float* hist_var, const float* hist_guide, const uint32_t* hist_ids,
                           float alpha_min, float sigma_depth, float normal_cos_min, uint32_t max_history, float* out_illum,
                           float* out_var);
/* Same with DEVICE pointers on `device`. */
int pbrhip_svgf_accumulate_device(int device, uint32_t width, uint32_t height, const float* d_rgba, const uint32_t* d_count,
                                  const float* d_albedo_hits, const uint32_t* d_feature_count, const float* d_motion, const float* d_guide,
                                  const uint32_t* d_ids, const float* d_hist_illum, const float* d_hist_var, const float* d_hist_guide,
                                  const uint32_t* d_hist_ids, float alpha_min, float sigma_depth, float normal_cos_min,
                                  uint32_t max_history, float* d_out_illum, float* d_out_var);

/* The filter; needs no scene.  illum / var: an accumulation's outputs (a negative var reads as 0); guide: that frame's guide, N = guide.xyz
 * as it is, z = guide.w, a pixel with guide.w == 0 is background; ids, albedo_hits + feature_count: as above, optional.  out_rgba: W*H*4,
 * colour | 1, zeros where the pixel is not live.  out_feedback (may be NULL): W*H*4, the illumination after the FIRST iteration | the
 * pixel's length (zeros where not live); handed in as the next frame's hist_illum it is the paper's feedback loop.
 * Per pair (p, q) of live pixels inside the image, q = p + (dx, dy) s: w_n = max(0, N_p . N_q)^(2^normal_squarings) and the depth term
 * x_z = |z_p - z_q| / ((sigma_depth z_p s) sqrt(dx dx + dy dy)) (0 when sigma_depth <= 0 or z_p == z_q) are pbrhip_denoise's; between two
 * background pixels w_n = 1, x_z = 0; a background pixel and a surface weigh 0; w_id = 1 when ids is NULL or ids[p] == ids[q], else 0.
 * Variance in, per live p with len_p = illum.w: len_p >= 4: v(0)_p = var_p.  Otherwise over the 7 x 7 window (s = 1, rows top to bottom,
 * each left to right, p itself with g = 1 first) with g = w_id w_n exp(-x_z):
 *   m = l_p + sum g (l_q - l_p) / sum g,   sigma2 = sum g ((l_q - m)(l_q - m)) / sum g,   v(0)_p = (sigma2 * 4) / len_p
 * with l = lum(illum.rgb): two passes over the window, not a difference of moments.
 * Iteration i = 0 .. iterations - 1, step s = 2^i, e(0) = illum.rgb: gv_p = sum k v(i)_q / sum k over the live pixels of the 3 x 3
 * window at distance 1 (whatever s; rows top to bottom), k = [1 2 1] x [1 2 1]; S_p = sigma_lum sqrt(gv_p) + PBRHIP_SVGF_LUM_EPS.  Over
 * pbrhip_denoise's 25 taps with its B3 weights h: w(p, p) = 1, else w = w_id w_n exp(-(x_z + x_l)), x_l = |lum(e_p) - lum(e_q)| / S_p
 * (0 when sigma_lum <= 0 or the two are equal), and with hw = (w_n exp(..)) h:
 *   e(i+1)_p = e_p + sum hw (e_q - e_p) / sum hw,   v(i+1)_p = sum (hw hw) v_q / (sum hw)(sum hw)
 * -- the denoiser's form: a constant neighbourhood returns to the bit.  out.rgb = e(iterations) max(a, 1e-3): the clamped value the
 * accumulation divided by -- deliberately not pbrhip_denoise's unclamped product, so that a surface of black albedo keeps its radiance.
 * iterations: 1 .. 8, 0 = PBRHIP_SVGF_ITERATIONS.  PBRHIP_SVGF_LUM_EPS is fixed: far above the rounding noise 2^-23 l of a constant region
 * for any l up to about 100 (such a region keeps weight 1), far below any real luminance step.  PBRHIP_SVGF_SIGMA_LUM is not the paper's
 * 4 but the optimum of the sweep over (1, 2, 4, 8, 16) on the orbiting Cornell sequence (profiles/README.md "SVGF": the error rises
 * with sigma_lum from 1 on; smaller values were not swept); sigma_depth and normal_squarings default to
 * PBRHIP_DENOISE_SIGMA_DEPTH and PBRHIP_DENOISE_NORMAL_SQUARINGS.  The sigmas are never read as "default": pass the macros.
 * PBRHIP_EINVAL: a NULL illum / var / guide / out_rgba, a NaN sigma, iterations > 8, normal_squarings > 16, a zero size, one of
 * albedo_hits / feature_count without the other, an output that is illum, guide or the other output.
 * Where the albedo hurts: a is estimated from each frame's own few samples, so at a pixel that an emitter of BLACK albedo covers partly
 * it changes from frame to frame between about 1e-3 and the neighbour's albedo, and a history e = c / 1e-3 multiplied by this frame's a
 * is wrong by orders of magnitude.  With such an emitter in view pass no albedo_hits / feature_count to either call (the colour itself
 * is then accumulated and filtered): DESIGN.md §17 has the figures of both on the Cornell box, whose light is one.  Or keep the albedo
 * and take the emitter's own radiance out of what is divided by it: pbrhip_emission_split below.
 * Not provided: a colour clamp against the current neighbourhood; |N . N| for hair tangents in the spatial weights (the filter has no
 * valid mark: two hairs of opposite tangent weigh 0); a multi-GPU twin. */
#define PBRHIP_SVGF_ITERATIONS 5
#define PBRHIP_SVGF_LUM_EPS 1e-4f
#define PBRHIP_SVGF_SIGMA_LUM 1.0f
int pbrhip_svgf_filter(int device, uint32_t width, uint32_t height, const float* illum, const float* var, const float* guide,
                       const uint32_t* ids, const float* albedo_hits, const uint32_t* feature_count, uint32_t iterations, float sigma_lum,
                       float sigma_depth, uint32_t normal_squarings, float* out_rgba, float* out_feedback);
/* Same with DEVICE pointers on `device`. */
int pbrhip_svgf_filter_device(int device, uint32_t width, uint32_t height, const float* d_illum, const float* d_var, const float* d_guide,
                              const uint32_t* d_ids, const float* d_albedo_hits, const uint32_t* d_feature_count, uint32_t iterations,
                              float sigma_lum, float sigma_depth, uint32_t normal_squarings, float* d_out_rgba, float* d_out_feedback);

/* ---- the first-hit emission layer: demodulate only the reflected light ----
 * The radiance the camera sees directly never touched an albedo, so it must not be divided by one.  The pipelines above become
 *   pbrhip_render -> pbrhip_render_features_emission -> pbrhip_render_motion -> pbrhip_scene_object_ids -> pbrhip_emission_split ->
 *   pbrhip_svgf_accumulate -> pbrhip_svgf_filter -> pbrhip_emission_merge,   or   pbrhip_emission_split -> pbrhip_denoise -> pbrhip_emission_merge,
 * the accumulation, the filter and the denoiser being the functions above, unchanged.
 *
 * The feature pass with one more buffer, in one trace.  albedo_hits, normal_depth and count are pbrhip_render_features' bit for bit, from
 * the same descriptor fields, with the same PBRHIP_RENDER_NO_CLEAR continuation, refusals and error codes; any of the four may be NULL.
 *   emission  W*H*4: sum of Le_first rgb | number of samples that added one
 * Le_first of a sample is what the renderer adds to its radiance at depth 0, with weight 1 and throughput 1 and no draw beyond the
 * camera's: on a hit that faces the ray (geometric and shading normal both against the direction) on a primitive of an area light, the
 * light's emission; on a miss in a scene with an environment, the environment's stored (scaled) texel in the ray's direction; otherwise
 * nothing.  Both are float32 sums in ascending pass order per pixel.  The layer does not depend on the materials: emission.rgb equals
 * the rgb sums pbrhip_render makes of the same scene with every material id PBRHIP_NONE, bit for bit.  It is also the emission AOV.
 * Not provided: an emission output for pbrhip_render_features_rays_device; the emission of deeper bounces. */
int pbrhip_render_features_emission(pbrhip_scene*, const pbrhip_render_desc*, float* albedo_hits, float* normal_depth, uint32_t* count,
                                    float* emission);
/* Same, into DEVICE buffers on the scene's device. */
int pbrhip_render_features_emission_device(pbrhip_scene*, const pbrhip_render_desc*, float* d_albedo_hits, float* d_normal_depth,
                                           uint32_t* d_count, float* d_emission);

/* Split and merge; they need no scene.  All arithmetic is float32, every operation rounded once.
 * Split, per pixel p (rgba / count: the RenderLayer's sums; emission: the layer above over the same passes):
 *   count == 0: out_rgba = (0, 0, 0, 0); otherwise d = rgba.rgb - emission.rgb per channel, out_rgba = (d > 0 ? d : +0, rgba.a)
 *   out_albedo_hits = (albedo_hits.rgb, (float)feature_count)
 * The subtraction is done on the sums, so what follows still divides by count.  With hits == feature_count the albedo of
 * pbrhip_denoise, pbrhip_svgf_accumulate and pbrhip_svgf_filter, a = (albedo.rgb + misses) / feature_count, becomes albedo.rgb /
 * feature_count: a miss (and an emitter) counts as BLACK, because its radiance is in the emission layer.  A pixel an emitter covers
 * with a fraction f of its samples has c = f Le + (1 - f) a_c e_c and a = (1 - f) a_c: (c - f Le) / a = e_c whatever f is.
 * albedo_hits, feature_count and out_albedo_hits are given all three or none.  out_rgba may be rgba, out_albedo_hits may be albedo_hits.
 * Merge, per pixel p (filtered_rgba: a filter's out_rgba of the split buffers; count: the RenderLayer's):
 *   count == 0: out_rgba = filtered_rgba; otherwise out.rgb = filtered.rgb + emission.rgb / (float)count, out.a = filtered.a
 * out_rgba may be filtered_rgba.
 * PBRHIP_EINVAL, before any device work: a zero size, a NULL required buffer, one or two of the albedo triple, out_albedo_hits being an
 * input other than albedo_hits (or out_rgba), an out_rgba that is an input other than rgba / filtered_rgba. */
int pbrhip_emission_split(int device, uint32_t width, uint32_t height, const float* rgba, const uint32_t* count, const float* emission,
                          const float* albedo_hits, const uint32_t* feature_count, float* out_rgba, float* out_albedo_hits);
/* Same with DEVICE pointers on `device`. */
int pbrhip_emission_split_device(int device, uint32_t width, uint32_t height, const float* d_rgba, const uint32_t* d_count,
                                 const float* d_emission, const float* d_albedo_hits, const uint32_t* d_feature_count, float* d_out_rgba,
                                 float* d_out_albedo_hits);
int pbrhip_emission_merge(int device, uint32_t width, uint32_t height, const float* filtered_rgba, const float* emission,
                          const uint32_t* count, float* out_rgba);
/* Same with DEVICE pointers on `device`. */
int pbrhip_emission_merge_device(int device, uint32_t width, uint32_t height, const float* d_filtered_rgba, const float* d_emission,
                                 const uint32_t* d_count, float* d_out_rgba);

/* ---- ray and nearest-point queries from device memory ----
 * What a simulation on the scene's GPU asks of a committed scene between its pbrhip_scene_update_*_device calls and refits, without a
 * round trip through the host: "what does this ray hit", "is this segment blocked", "which primitive is nearest to this point".
 *
 * Alignment: the kernels read and write 16 bytes at a time, so d_rays, d_points, d_ident and d_closest must be 16-byte aligned device
 * pointers (what hipMalloc returns, and any float32 tensor of shape (n, 8) or (n, 4) that starts its allocation, is); d_hits needs
 * 4 bytes, d_occluded none.  A pointer that is not is refused with PBRHIP_EINVAL before any device work.
 *
 * Ray queries.  d_rays: n pbrhip_ray in device memory of the scene's device; `stream`: the stream they are produced on -- they are read
 * only after the work already enqueued there, and the call returns when the outputs are written (pbrhip_scene_object_ids_device's rule).
 *   d_ident  4 words per ray: slot, then the bits of u, v, t; a miss: (PBRHIP_NONE, 0, 0, 0).  pbrhip_render_motion's identity format:
 *            pbrhip_scene_object_ids_device takes it as it is.
 *   d_hits   bit for bit what pbrhip_trace_closest writes for the same ray.
 *   d_occluded  one byte per ray, what pbrhip_trace_any writes.
 * Either of d_ident and d_hits may be NULL.  A ray is traced as given: tmin and tmax are honoured, dir is not renormalised.  An inactive
 * ray (pbrhip_render_rays' rule: a NaN among its eight numbers, an infinite origin or direction component, a zero direction, tmin < 0 or
 * !(tmax >= tmin)) is a miss / not occluded, with no fault.  The kernels run the production traversal on the tree the scene's render
 * walks (PBRHIP_WIDE=0 selects the binary tree); the results do not depend on the tree.
 * PBRHIP_EINVAL ("NULL" in pbrhip_last_error): a NULL scene, or with n > 0 NULL rays or no output; PBRHIP_EINVAL: n >= 2^31 -- both before
 * any device work; PBRHIP_ESTATE: an uncommitted or stale scene; PBRHIP_EOVERFLOW: a traversal stack overflow; n == 0: PBRHIP_OK. */
int pbrhip_trace_closest_device(pbrhip_scene*, const void* d_rays, size_t n, void* stream, uint32_t* d_ident, pbrhip_hit* d_hits);
int pbrhip_trace_any_device(pbrhip_scene*, const void* d_rays, size_t n, void* stream, uint8_t* d_occluded);

/* Nearest-point queries.  Per query (p, max_dist): the primitive of smallest distance D2 among those with D2 <= max_dist * max_dist
 * (rounded once; max_dist = +inf: no bound); equal D2 goes to the smaller canonical primitive id (the ray contract's tie rule).
 *   ident    4 words per query: slot, then the bits of u, v, sqrtf(D2); a miss: (PBRHIP_NONE, 0, 0, 0)
 *   closest  4 floats per query: the closest point q, then D2; a miss: zeros
 * Either may be NULL.  A query with a NaN or infinite coordinate, or max_dist NaN or below 0, is inactive: a miss.
 * D2 is defined exactly, in float32 with every operation rounded once (DESIGN.md §19 has it operation by operation):
 *   segment (x, y): e = y - x, t = clamp(dot(p - x, e) / dot(e, e), 0, 1) (0 when dot(e, e) is not > 0), q = x + t e, |p - q|^2
 *   triangle (a, b, c): d2_raw = the minimum of the segments ab, bc, ca in that order (a strict < replaces) and, last and again by strict <,
 *     of the plane term (h / nn) h, n = cross(b - a, c - a), nn = dot(n, n), h = dot(p - a, n), which applies when nn > 0 and
 *     dot(cross(y - x, p - x), n) >= 0 for the three edges; q = the closest point of the winning feature (the plane's: p - (h / nn) n);
 *     (u, v) = its barycentrics of b and c (ab: (t, 0); bc: (1 - t, t); ca: (0, 1 - t); plane: the ca and ab sign terms over nn)
 *   curve piece: the segment between its end points -- the centre line; the radius is ignored --, u = (sub + t) / 4, v = 0
 *   D2 = max(d2_raw, L) with L the squared distance from p to the primitive's own box (the one the intersection contract validates
 *     with, widened the same way): every stored box of either tree contains that box, so a traversal that skips a box only when its own
 *     squared distance exceeds the best D2 cannot skip the answer, and the result is a property of (point, primitive set) alone: it does
 *     not depend on builder, tree, refit or visiting order.
 * Domain: nn is fourth order in a triangle's edge length, so float32 bounds the scale of a scene.  The distance is within 9.08 units of
 * 2^-24 (largest |coordinate| + distance) of its float64 value for edge length x query distance from about 1e-17 to 1e18 -- scenes whose
 * triangles have edges of 0.3 s and whose queries lie up to 3 s away, s = 1e-8 .. 1e9 -- and at offsets up to 1e7, under anisotropic
 * scales of 1e7 between axes and on flat scenes (measured: at most 5.10 units; DESIGN.md §19 "Domain").  A decade outside it nn
 * underflows or overflows: the answer is still the contract's, bit for bit, but no longer the distance.
 * The device variant orders the read of d_points behind `stream` as above.  Errors as the ray queries'.
 * Not provided: the ribbon's radius, a multi-GPU twin, asynchronous return.  (Signed distance, all-hits ray queries and the K nearest
 * primitives of a point: below.) */
typedef struct {
  float p[3];
  float max_dist;
} pbrhip_point; /* 16 bytes */
int pbrhip_nearest_point(pbrhip_scene*, const pbrhip_point* points, size_t n, uint32_t* ident, float* closest);
int pbrhip_nearest_point_device(pbrhip_scene*, const void* d_points, size_t n, void* stream, uint32_t* d_ident, float* d_closest);

/* ---- signed distance ----
 * "How far is the nearest surface, and on which side of it am I": the nearest-point query above with a sign.  ident and closest are
 * pbrhip_nearest_point_device's, byte for byte, on the same points; the sign comes from the angle-weighted pseudonormal (Baerentzen &
 * Aanaes 2005) of the FEATURE of the nearest triangle the closest point lies on:
 *   the winning segment ab, bc or ca with 0 < t < 1: that edge; with its clamped t at 0 or 1 (a segment without length has t = 0): the
 *   vertex at that end; the plane term: the face.
 *   sd       4 floats per query: the feature's pseudonormal N, then the signed distance: sqrtf(D2) when dot(p - q, N) >= 0, -sqrtf(D2)
 *            when it is < 0.  Outside is positive.  A curve piece has no normal: N = 0, a positive distance.  A miss or an inactive
 *            query: zeros (ident and closest as above).
 * Pseudonormals.  A face's unit normal is n / sqrtf(dot(n, n)), n = cross(b - a, c - a) of the world-space corners in the order the
 * mesh indexes them; a face whose dot(n, n) is not > 0 contributes nothing.  An edge's: the sum of the unit normals of the faces of the
 * same object that have it; a vertex's: the sum of (corner angle x unit normal) over the faces of the same object at it, the angle
 * atan2(|e1 x e2|, e1 . e2) between the face's two edges there; both sums in ascending canonical primitive id, normalised, or zero if
 * their length is not > 0.  float32, every operation rounded once: the table depends on the model alone, not on builder or tree.
 * Vertex identity: two corners are the same vertex when they belong to the same object -- the same instance and geometry -- and carry
 * the same entry of the mesh's vertex_ids.  Equal positions under different indices are NOT welded: a mesh that duplicates its vertices
 * along a seam has boundary edges there.  Since normals are taken from world-space corners, an instance whose transform mirrors
 * (negative determinant) is inside-out: its signs are flipped.
 * The sign is a guarantee only where the nearest object is a closed, consistently oriented manifold; pbrhip_sd_info reports what the
 * scene has.  An open mesh still works: a boundary edge carries its one face's normal.
 * Domain: pbrhip_nearest_point's (edge length x query distance from about 1e-17 to 1e18), which the table's own dot(n, n) shares: on closed
 * shapes at the uniform scales 1e-8 .. 1e9 and at an offset of 1e4 the table stays within its rounding bound and the sign is the
 * float64 winding number's at every point farther from the surface than the rounding of q (DESIGN.md §20 "Domain").
 * The table is built on the device at the first of these calls after a commit or a refit; a scene that never calls them allocates and
 * launches nothing for it.  A replica (pbrhip_scene_replicate) holds no geometry: PBRHIP_ESTATE.
 * Stream ordering, the 16-byte alignment of d_points, d_ident, d_closest and d_sd, refusals and error codes: pbrhip_nearest_point_device's.
 * Any of the three outputs may be NULL, not all.
 * Grid: the same query at p = origin + (float)(i, j, k) * spacing (multiply, then add, each rounded once) for i < dims[0], j < dims[1],
 * k < dims[2], all with max_dist; d_sd: dims[2] x dims[1] x dims[0] floats (x fastest; 4-byte aligned), the signed distance alone, 0
 * where nothing lies within max_dist.  A dims of 0: PBRHIP_OK and nothing written; 2^31 points or more: PBRHIP_EINVAL.
 * Not provided: the generalized winding number as a sign method, welding by position, the ribbon's radius, a multi-GPU twin. */
typedef struct {
  uint32_t triangles;           /* triangle slots of the scene */
  uint32_t vertices;            /* distinct (object, index) vertices they use */
  uint32_t edges_manifold;      /* exactly two faces, running along the edge in opposite directions */
  uint32_t edges_boundary;      /* one face */
  uint32_t edges_nonmanifold;   /* three or more faces */
  uint32_t edges_inconsistent;  /* two faces running along the edge in the same direction */
  uint64_t table_bytes;         /* device memory of the table and its lists */
  double topology_ms, table_ms; /* host time of the lists (once per commit); device time of the last table build */
} pbrhip_sd_info;
int pbrhip_scene_signed_distance_info(pbrhip_scene*, pbrhip_sd_info* out);
int pbrhip_signed_distance(pbrhip_scene*, const pbrhip_point* points, size_t n, uint32_t* ident, float* closest, float* sd);
int pbrhip_signed_distance_device(pbrhip_scene*, const void* d_points, size_t n, void* stream, uint32_t* d_ident, float* d_closest, float* d_sd);
int pbrhip_signed_distance_grid_device(pbrhip_scene*, const float origin[3], const float spacing[3], const uint32_t dims[3], float max_dist,
                                       void* stream, float* d_sd);
/* test hook: the table as the device holds it.  Per slot seven rows of four floats -- ab, bc, ca, a, b, c, face; xyz and 0 --, zeros for
 * a curve slot; out: *num_slots x 28 floats (NULL: only the count).  Builds the table if needed. */
int pbrhip_scene_read_pseudonormals(pbrhip_scene*, float* out, uint32_t* num_slots);

/* ---- all-hits ray queries ----
 * "Everything this ray hits, in order": several returns per lidar beam, the thickness of material along a ray, an inside / outside test
 * by crossing parity where the pseudonormal sign above is no guarantee, depth peeling in one launch.  Peeling with
 * pbrhip_trace_closest_device -- K calls, tmin advanced to the last t -- costs K traversals and loses every hit but one wherever two
 * primitives are hit at the same t (exact duplicates, coplanar overlaps); this query does not.
 * A UNIT is what a leaf of the tree tests once: a triangle, or one of the four linear pieces of a curve's cubic.  A unit's hit is
 * ACCEPTED exactly when the closest-hit traversal could accept it: the primitive test passes, tmin < t <= tmax, and t lies in the interval
 * in which the ray crosses the unit's own box (the validation of the intersection contract) -- the same functions, the same
 * operations, the same bits of t, u, v.  For a ray let H be the accepted hits of all units of the scene, ordered by the key
 *   (t ascending; then the canonical primitive id -- (instance, geometry, primitive) order, what PBRHIP_ID_PRIMITIVE reports -- ascending;
 *    then u ascending).
 * Two pieces of one cubic share an id and can tie in t: they differ in u, the curve parameter.  Two hits equal in all three are the same
 * record.  Outputs for ray i with max_hits = K:
 *   count[i]          |H|: every accepted hit, NOT capped by K
 *   ident[i * K + j]  4 words each, j < K: for j < min(|H|, K) the j-th hit of that order in pbrhip_trace_closest_device's identity format
 *                     (slot, then the bits of u, v, t; a curve hit is named by its slot as there; pbrhip_scene_object_ids_device takes
 *                     the n * K entries as they are); every remaining entry (PBRHIP_NONE, 0, 0, 0).
 * So ident[i * K + 0] equals pbrhip_trace_closest_device's d_ident[i] byte for byte, for every ray and every K >= 1, and the result is a
 * property of (ray, primitive set) alone: it does not depend on builder, tree (PBRHIP_WIDE=0 / 1), refit or visiting order.  An inactive
 * ray (the ray queries' rule above: a NaN among its eight numbers, an infinite origin or direction component, a zero direction, tmin < 0
 * or !(tmax >= tmin)) has count 0 and a row of misses, with no fault.
 * max_hits is in [0, PBRHIP_ALL_HITS_MAX].  Either output may be NULL, not both: max_hits == 0 requires count and ignores ident;
 * max_hits > 0 with ident == NULL is a pure count as well.  With count the traversal enters every box the ray crosses in [tmin, tmax];
 * without it the interval shrinks to the K-th hit once the list is full (K = 1: the closest-hit traversal), so ask for the count only
 * when it is wanted.  The list is kept in the ray's row of ident while the kernel runs.
 * Stream ordering, the 16-byte alignment of d_rays and d_ident (d_count: 4 bytes), refusals and error codes are
 * pbrhip_trace_closest_device's: PBRHIP_EINVAL before any device work for a NULL scene, with n > 0 NULL rays or no usable output
 * ("NULL" in pbrhip_last_error), max_hits > PBRHIP_ALL_HITS_MAX, n >= 2^31 or n * max_hits >= 2^31 ("too many"); PBRHIP_ESTATE: an
 * uncommitted or stale scene; PBRHIP_EOVERFLOW: a traversal stack overflow; n == 0: PBRHIP_OK.  The host variant stages rays and outputs
 * through device memory as pbrhip_nearest_point does.
 * Not provided: more than PBRHIP_ALL_HITS_MAX listed hits per ray (count says how many there are; peel on from the last t), any-hit
 * filters or callbacks, a multi-GPU twin, asynchronous return. */
#define PBRHIP_ALL_HITS_MAX 32u
int pbrhip_trace_all(pbrhip_scene*, const pbrhip_ray* rays, size_t n, uint32_t max_hits, uint32_t* count, uint32_t* ident);
int pbrhip_trace_all_device(pbrhip_scene*, const void* d_rays, size_t n, uint32_t max_hits, void* stream, uint32_t* d_count,
                            uint32_t* d_ident);

/* ---- k-nearest queries ----
 * "Every primitive within my contact radius, or the few nearest": collision and contact candidates, attachment of hair roots or cloth to
 * a moving body, smoothing over neighbours.  pbrhip_nearest_point above gives the one nearest; this gives the K nearest and how many lie
 * within the radius, in one launch, without reading the slots back.
 * A UNIT is what a leaf of the tree tests once: a triangle, or one of the four linear pieces of a curve's cubic.  For a query
 * (p, max_dist) a unit's candidate is pbrhip_nearest_point's D2, u, v, q -- the same functions, the same operations, the same bits, the
 * validation clamp D2 = max(d2_raw, L) included.  C(p) is the set of units with D2 <= max_dist * max_dist (rounded once; a NaN never
 * qualifies; max_dist = +inf: no bound), ordered by the key
 *   (D2 ascending; then the canonical primitive id -- what PBRHIP_ID_PRIMITIVE reports -- ascending; then sub ascending),
 * sub being the piece's index inside its cubic, 0 for a triangle, so the order is total.  (This library numbers the canonical ids per
 * unit, in (instance, geometry, primitive, sub) order: the id alone decides, and among the pieces of one cubic it decides as sub would.
 * u could not be the last key as in pbrhip_trace_all: pieces k and k + 1 of a cubic meet in a joint, and a point nearest to that joint
 * gives both the same D2 and the same u = (k + 1) / 4.)  Outputs for query i with max_k = K:
 *   count[i]            |C(p)|: every unit within the radius, NOT capped by K
 *   ident[i * K + j]    4 words each, j < K: for j < min(|C|, K) the j-th unit of that order in pbrhip_nearest_point's format (slot, then
 *                       the bits of u, v, sqrtf(D2); pbrhip_scene_object_ids_device takes the n * K entries as they are); every
 *                       remaining entry (PBRHIP_NONE, 0, 0, 0)
 *   closest[i * K + j]  4 floats each: the listed unit's closest point q, then D2; every remaining entry zeros
 * THE ORDER IS D2's, NOT THE DISTANCE's: sqrtf merges distinct D2, so two successive entries may show equal distances while their D2
 * -- and hence their order -- differ (on the 430-triangle test soup 35 of 3000 queries have such a pair among their first 33 entries).
 * A caller who needs the strict order reads closest's w.
 * Entry 0 is pbrhip_nearest_point's answer byte for byte: that query gives a shared minimum to the smaller canonical id as well, two
 * pieces of one cubic at their joint included.  The result is a property of (point, primitive set) alone: it does
 * not depend on builder, tree (PBRHIP_WIDE=0 / 1), refit or visiting order.  An inactive query (a NaN or infinite coordinate, max_dist
 * NaN or below 0) has count 0 and rows of misses, with no fault.
 * max_k is in [0, PBRHIP_K_NEAREST_MAX].  Any output may be NULL, with two restrictions: closest requires ident (the list lives in the
 * ident rows while the kernel runs), and max_k == 0 requires count (ident and closest are then ignored); max_k > 0 with ident == NULL is
 * a pure count as well.  Without count the traversal's bound shrinks to the K-th entry's D2 once the list is full (K = 1: the
 * nearest-point traversal); with count it stays max_dist^2 and every box within the radius is entered, so ask for the count only when it
 * is wanted.  count with max_dist = +inf is allowed: it counts every unit whose D2 is not a NaN, at the price of a walk of the whole tree.
 * Stream ordering, the 16-byte alignment of d_points, d_ident and d_closest (d_count: 4 bytes), refusals and error codes are
 * pbrhip_trace_all_device's: PBRHIP_EINVAL before any device work for a NULL scene, with n > 0 NULL points or no usable output, closest
 * without ident ("NULL" in pbrhip_last_error), max_k > PBRHIP_K_NEAREST_MAX ("max_k"), n >= 2^31 or n * max_k >= 2^31 ("too many"), a
 * misaligned device pointer ("aligned"); PBRHIP_ESTATE: an uncommitted or stale scene or a replica; PBRHIP_EOVERFLOW: a traversal stack
 * overflow; n == 0: PBRHIP_OK.  The host variant stages points and outputs through device memory as pbrhip_trace_all does.
 * Not provided: more than PBRHIP_K_NEAREST_MAX listed units per query (count says how many there are), the ribbon's radius, a multi-GPU
 * twin, asynchronous return, filters or callbacks. */
#define PBRHIP_K_NEAREST_MAX 32u
int pbrhip_k_nearest(pbrhip_scene*, const pbrhip_point* points, size_t n, uint32_t max_k, uint32_t* count, uint32_t* ident, float* closest);
int pbrhip_k_nearest_device(pbrhip_scene*, const void* d_points, size_t n, uint32_t max_k, void* stream, uint32_t* d_count,
                            uint32_t* d_ident, float* d_closest);

/* ---- multi-GPU (new: the reference has one process and std::threads, render.cc:203-238) ----
 * Pixels are independent, so the only exchange is the RenderLayer at the end of a frame: rank r renders the pixel blocks
 * with index % world == r (pbrhip_render_desc.tile_rank / tile_world / shard_block) into a zeroed full-size layer, then the
 * layers are combined on one rank.  Disjoint blocks + zeros: the combined frame is bit-identical to the one-GPU frame. */

/* (1) one process, several GPUs: scenes[i] is a committed copy of the same scene on its own device (pbrhip_scene_replicate;
 * several scenes may share a device).  One host thread per scene renders rank desc->tile_rank * n + i of
 * desc->tile_world * n; the shards are then copied device-to-device (xGMI peer copies: only the blocks a rank rendered
 * travel) into scenes[0]'s layer and from there to the host.  cancel / finish_pass as in pbrhip_render, except that the
 * devices of a cancelled call stop at their own pass counts: *finish_pass = the passes complete on EVERY device (the
 * minimum), a device that was ahead keeps its further passes in its pixels, and `count` says per pixel how many it holds;
 * stats: NULL or n records. */
int pbrhip_render_multi(pbrhip_scene* const* scenes, uint32_t n, const pbrhip_render_desc*,
                        const volatile unsigned char* cancel, float* rgba, uint32_t* count, size_t* finish_pass,
                        pbrhip_render_stats* stats);
/* A committed scene's copy on another device (device memory is copied device-to-device: no second ingestion, no second
 * BVH build); what `pbrlab-hip-cli --gpus N` calls per extra GPU. */
int pbrhip_scene_replicate(const pbrhip_scene* src, int device, pbrhip_scene** out);

/* (2) one process per GPU (torch.distributed / MPI launchers): an RCCL communicator inside the library.
 * pbrhip_comm_unique_id: ncclGetUniqueId on one rank; the launcher hands the 128 bytes to every rank.
 * pbrhip_comm_create: ncclCommInitRank on the device selected with pbrhip_set_device (collective: every rank calls it). */
#define PBRHIP_COMM_ID_BYTES 128
typedef struct pbrhip_comm pbrhip_comm;
int pbrhip_comm_unique_id(unsigned char id[PBRHIP_COMM_ID_BYTES]);
int pbrhip_comm_create(pbrhip_comm** out, const unsigned char id[PBRHIP_COMM_ID_BYTES], int rank, int world);
int pbrhip_comm_destroy(pbrhip_comm*);
/* ncclReduce(sum) of rgba (f32) and count (u32) to `root`, in place, in one RCCL group: what SURVEY 8e specifies.  Works
 * for any layers (e.g. different passes of the same pixels on different ranks).  Blocking. */
int pbrhip_comm_reduce_layer(pbrhip_comm*, float* d_rgba, uint32_t* d_count, size_t num_pixels, int root);
/* The same result for layers rendered with (tile_rank, tile_world) = (rank, world) of the communicator and `desc`'s
 * width / height / shard_block: a reduce whose zero terms do not travel.  Every rank packs the pixels of its own blocks
 * (20 bytes per pixel) and sends them straight to `root` (ncclSend / ncclRecv in one group: xGMI is point-to-point, so
 * the N - 1 shards arrive over N - 1 different links at once), root scatters them into its layer.  Blocking. */
int pbrhip_comm_gather_layer(pbrhip_comm*, pbrhip_scene*, const pbrhip_render_desc* desc, float* d_rgba,
                             uint32_t* d_count, int root);

/* Raytracer::FirstHitTrace1 / AnyHit1 (src/raytracer/raytracer.h:95-111, raytracer_impl.cc:268-287) over an
 * array of rays: test hooks for hit-index parity */
int pbrhip_trace_closest(pbrhip_scene*, const pbrhip_ray* rays, size_t n, pbrhip_hit* hits);
int pbrhip_trace_any(pbrhip_scene*, const pbrhip_ray* rays, size_t n, uint8_t* occluded);
/* The GPU builder (PBRHIP_BVH_GPU_LBVH) on n bare boxes lo / hi (3 floats each) of kinds[i] (0 triangle, 1 curve piece), without a
 * scene: a test hook.  nodes_out (host) receives max(n - 1, 1) traversal nodes of 64 bytes (lo[3][2], hi[3][2], c0, c1, pad[2]),
 * order_out the primitive of every leaf slot, depth_out the stack depth a traversal needs.  It returns what the builder made however
 * deep it is: replacing a tree deeper than the traversal stack by a host-built one is pbrhip_scene_commit's business.  The tree is
 * defined exactly ("The tree, exactly"): per axis c = 0.5f * (lo + hi), cell = (uint)(q * 2097151.0f) with
 * q = (c - min c) / (max c - min c) clamped to [0, 1] (0 on a flat axis), every step rounded to single precision; a 63-bit key with x
 * in the highest bit of each triple; a stable sort; the radix tree over (key, position), equal keys continuing with the 32-bit
 * positions (prefix 64 + clz(i ^ j)); node 0 the root, the children of a node that splits after position g being nodes g and g + 1;
 * a subtree of at most two primitives of one kind stored as a leaf reference of its parent; boxes widened like every stored box;
 * depth = height of the root + 1.  Boxes whose lo + hi overflows, or that are not finite, are outside that definition.
 * NULL arguments or n >= 2^27: PBRHIP_EINVAL.  n == 0: PBRHIP_OK, nothing is written. */
int pbrhip_lbvh_build(int device, const float* lo, const float* hi, const uint8_t* kinds, uint32_t n, void* nodes_out,
                      uint32_t* order_out, uint32_t* depth_out);
/* Builder GPU_LBVH_WIDE without a scene: a test hook.  lo / hi / kinds as for pbrhip_lbvh_build; slots: n records of 64 bytes, one per
 * PRIMITIVE (four 16-byte words as a scene's slots: a triangle's corners, routing bits in .w of the third word; a curve piece's two end
 * points xyzr, then its index in the cubic as the bits of the third word's .x).  sizes_out[6] receives: Q nodes, 16-byte words of
 * triangle leaves, points, stack need, flags (1: every record index fits its reference, 2: every node was quantised), depth of the
 * binary tree.  With qnodes_out == NULL only sizes_out (but the stack need) is written: call once for the sizes, then again with
 * nodes_out (max(n - 1, 1) x 64 B), order_out (n), qnodes_out (sizes[0] x 64 B), tri_out (sizes[1] x 16 B), pts_out (sizes[2] x 16 B)
 * and hit_out (sizes[2] words).  No fallback: whatever the collapse made is returned.  n == 0: sizes all zero. */
int pbrhip_qtree_collapse(int device, const float* lo, const float* hi, const uint8_t* kinds, const void* slots, uint32_t n,
                          void* nodes_out, uint32_t* order_out, void* qnodes_out, void* tri_out, void* pts_out, uint32_t* hit_out,
                          uint32_t* sizes_out);
/* pbrhip_scene_refit's device work without a scene: a test hook.  slots: n x 64 B, the NEW slots in leaf order; nodes_inout: the
 * max(n - 1, 1) binary nodes; qnodes_inout (num_qnodes x 64 B), tri_inout (tri_words x 16 B; tri_pairs: TriPair records, else 48-byte
 * slots), pts_inout (num_points x 16 B) and hit (num_points words): the Q tree over them as pbrhip_qtree_collapse returns it;
 * qnodes_inout == NULL: the binary tree only.  Uploads, runs the kernels pbrhip_scene_refit runs (plan, leaf records, both trees) and
 * downloads.  A node that cannot be quantised or an index out of range: PBRHIP_EHIP.  n == 0: PBRHIP_OK, nothing is written. */
int pbrhip_tree_refit(int device, uint32_t n, const void* slots, void* nodes_inout, void* qnodes_inout, uint32_t num_qnodes,
                      void* tri_inout, uint32_t tri_words, int tri_pairs, void* pts_inout, const uint32_t* hit, uint32_t num_points);
/* The camera ray the renderer traces for sample `pass` of pixel (x, y) of a width x height image (x_y_pass: n triples), evaluated on the
 * device: the user camera when one is set, else the reference's (which needs a committed scene: its box).  For tests and picking
 * (the ray of a pixel, for pbrhip_trace_closest). */
int pbrhip_camera_rays(pbrhip_scene*, uint32_t width, uint32_t height, uint64_t seed_seq, const uint32_t* x_y_pass, size_t n, pbrhip_ray* rays);

/* The device's leaf functions on arrays of inputs -- a test hook like the two above: what the kernels compute for the generator
 * (src/random/rng.h), the fast math of the hair BSDF (src/pbrlab_math.h:135-344), Fresnel and the MIS weight (closure-util.h,
 * sampling-utils.h), the Lambert / sphere / triangle samplers (closure/lambert.h, sampler/sampling-utils.h), GGX eval and sample
 * (closure/microfacet-ggx.h:164-286) and the hair BSDF (closure/energy-conserving-hair-bsdf.h:295-572), so that they can be compared
 * with outputs of the reference's own headers.  n items; item i reads in_words floats at in + i * in_words and writes out_words at
 * out + i * out_words (host memory; integers travel as their bits):
 *   RNG          in: initstate lo, hi, initseq lo, hi            out: out_words draws
 *   FASTMATH     in: function (0 sin 1 cos 2 exp 3 log 4 atan2(x, y) 5 asin 6 exp2 7 log2 8 / 9 sincos' sine / cosine), x, y   out: 1
 *   FRESNEL      in: cos, eta -> 1        MIS: sampled pdf, other pdf -> 1
 *   LAMBERT      in: u0, u1 -> wi[3], f, pdf     SPHERE: u1, u2 -> v[3]     TRIANGLE: u1, u2 -> a, b
 *   GGX_EVAL     in: wi[3], wo[3], ax, ay, distrib -> f, pdf        GGX_SAMPLE: wo[3], ax, ay, u0, u1, distrib -> wi[3], f, pdf
 *   HAIR_EVAL    in: wi[3], wo[3], params[23] -> f[3], pdf           HAIR_SAMPLE: wo[3], params[23], us[4] -> wi[3], f[3], pdf
 *   (params: h, v[4], s, sigma_a[3], eta, alpha, tints[4][3], transparent_scale)
 * and the random walk's leaves (src/shader/random-walk-sss.h, cycles-principled-shader.cc:326-365), held to a float64 model of the text:
 *   SSS_MEDIUM   in: the 25 words of a pbrhip_principled_param -> enable_diffuse, enable_subsurface, subsurface weight[3], albedo[3], radius[3],
 *                diffuse weight[3], sigma_t[3], sigma_s[3], first walk throughput[3]: ParamToBsdf, then the medium as commit hoists it
 *   SSS_DISTANCE in: throughput[3], sigma_s[3], sigma_t[3], u0, u1 -> t, channel pdf[3] (albedo computed inside) | t, channel pdf[3] (albedo
 *                handed in): SampleScatterDistance
 *   SSS_SCATTER  in: org[3], dir[3], sigma_t[3], sigma_s[3], throughput[3], t_scatter, step, generator state lo, hi, increment lo, hi
 *                -> alive, org[3], dir[3], throughput[3], t_scatter, step, state lo, hi, 1 when the step kernel's and the walk kernel's way
 *                of calling it agree in every bit: one scattering event of the walk (random-walk-sss.h:343-361, :287-314); a walk that
 *                ends leaves its state as it came */
enum {
  PBRHIP_LEAF_SSS_MEDIUM = 11, PBRHIP_LEAF_SSS_DISTANCE = 12, PBRHIP_LEAF_SSS_SCATTER = 13,
  PBRHIP_LEAF_RNG = 0, PBRHIP_LEAF_FASTMATH = 1, PBRHIP_LEAF_FRESNEL = 2, PBRHIP_LEAF_MIS = 3, PBRHIP_LEAF_LAMBERT = 4, PBRHIP_LEAF_SPHERE = 5,
  PBRHIP_LEAF_TRIANGLE = 6, PBRHIP_LEAF_GGX_EVAL = 7, PBRHIP_LEAF_GGX_SAMPLE = 8, PBRHIP_LEAF_HAIR_EVAL = 9, PBRHIP_LEAF_HAIR_SAMPLE = 10
};
int pbrhip_leaf_eval(uint32_t op, const float* in, size_t n, uint32_t in_words, float* out, uint32_t out_words);
/* Texture::FetchFloat3 (src/texture.cc:43-68 -> BilinearFilter, src/image-utils.cc:99-167) of texture `texture_id` of a committed
 * scene at n coordinates uv[2 * i], uv[2 * i + 1] -> rgb[3 * i ..]: the fetch of the textured shading kernels, as a test hook */
int pbrhip_texture_fetch(pbrhip_scene*, uint32_t texture_id, const float* uv, size_t n, float* rgb);

/* CreateTiles (src/render-tile.cc:29-41): out = sx,tx,sy,ty per tile (may be NULL to query the count) */
int pbrhip_create_tiles(uint32_t width, uint32_t height, uint32_t* out_sx_tx_sy_ty, uint32_t* num_tiles);

#ifdef __cplusplus
}
#endif
#endif /* PBRHIP_H_ */
