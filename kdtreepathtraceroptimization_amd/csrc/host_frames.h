// host_frames.h -- spp-sharded frames across GPUs (kdpt_comm_*, kdpt_render_frames), RCCL loaded at run time, and
// kdpt_destroy (which releases the communicator).  The in-process group of contexts (kdpt_group_*, and
// kdpt_render_sharded on top of it) is host_group.h, which uses this section's frame helpers.
//
// A host section of kdpt_runtime.hip's translation unit, not a stand-alone header: kdpt_runtime.hip includes it
// after host_output.h.  Host code only: no kernel is defined here (the kernels_*.h sections hold them), and
// tests/test_stream_discipline.py and tests/test_resource_ownership.py read every host section.
#pragma once

// Multi-GPU: samples per pixel sharded across GPUs (the reference renders one GPU's
// iterations in pathtrace(), src/pathtrace.cu:2405-2635).  Frame f covers global iterations f * spp + 1 ..
// (f + 1) * spp; rank r of N renders those with (iteration - 1 - f * spp) % N == r, in order, into its frame
// buffer, and one reduce (sum, to rank 0) per frame combines them -- the path's only exchange step.  Every
// iteration-dependent behaviour (RNG seeds, iteration 2's sort, cacherays) uses the global numbers.
//
// The reduce is RCCL's (ncclReduce over xGMI, one communicator rank per context; multi-process:
// kdpt_comm_init, one process per GPU) or, inside one process (kdpt_render_sharded), either RCCL
// (ncclCommInitAll) or a peer-copy reduce on device 0 that adds the ranks' frames in rank order (also usable
// with several contexts on one device, which RCCL refuses).  RCCL is loaded at run time (dlopen): the library
// has no link-time dependency on it, and a process that already holds it (torch) shares that copy.  Each
// context queues its frames' reduces and rank 0's image adds on a reduce stream of its own, which waits for
// the frame's last add (the batch streams' add chain), so frames stay in flight: frame f + 1's iterations run
// while frame f is reduced.
namespace {

struct Rccl {
  ncclResult_t (*getUniqueId)(ncclUniqueId*);
  ncclResult_t (*commInitRank)(ncclComm_t*, int, ncclUniqueId, int);
  ncclResult_t (*commInitAll)(ncclComm_t*, int, const int*);
  ncclResult_t (*commDestroy)(ncclComm_t);
  ncclResult_t (*reduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, int, ncclComm_t, hipStream_t);
  ncclResult_t (*groupStart)();
  ncclResult_t (*groupEnd)();
  const char* (*errorString)(ncclResult_t);
};

const Rccl* rccl() {
  static std::once_flag once;
  static Rccl r{};
  static bool ok = false;
  std::call_once(once, [] {
    void* h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!h) h = dlopen("/opt/rocm/lib/librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!h) return;
    r.getUniqueId = (decltype(r.getUniqueId))dlsym(h, "ncclGetUniqueId");
    r.commInitRank = (decltype(r.commInitRank))dlsym(h, "ncclCommInitRank");
    r.commInitAll = (decltype(r.commInitAll))dlsym(h, "ncclCommInitAll");
    r.commDestroy = (decltype(r.commDestroy))dlsym(h, "ncclCommDestroy");
    r.reduce = (decltype(r.reduce))dlsym(h, "ncclReduce");
    r.groupStart = (decltype(r.groupStart))dlsym(h, "ncclGroupStart");
    r.groupEnd = (decltype(r.groupEnd))dlsym(h, "ncclGroupEnd");
    r.errorString = (decltype(r.errorString))dlsym(h, "ncclGetErrorString");
    ok = r.getUniqueId && r.commInitRank && r.commInitAll && r.commDestroy && r.reduce && r.groupStart &&
         r.groupEnd && r.errorString;
  });
  return ok ? &r : nullptr;
}

#define RCCL_TRY(R, x)                                                                 \
  do {                                                                                 \
    const ncclResult_t e_ = (x);                                                       \
    if (e_ != ncclSuccess) return fail(KDPT_ERR_HIP, std::string("rccl: ") + (R)->errorString(e_)); \
  } while (0)

int reduce_spin(kdpt_ctx* c, hipStream_t st) {
  if (!(c->frames.reduce_spin_us > 0)) return KDPT_OK;
  const unsigned long long ticks = (unsigned long long)(c->frames.reduce_spin_us * c->wall_khz / 1000.0);
  hipLaunchKernelGGL(k_spin, dim3(1), dim3(64), 0, st, ticks);
  HIP_TRY(hipGetLastError());
  return KDPT_OK;
}

void release_comm(kdpt_ctx* c) {
  const Rccl* R = c->frames.comm && c->frames.owns_comm ? rccl() : nullptr;
  if (R) (void)R->commDestroy((ncclComm_t)c->frames.comm);
  c->frames.comm = nullptr;
  c->frames.owns_comm = false;
}

// Floats of a frame buffer: S alone, or, for a rank of a group whose frames carry second moments, S then Q in one
// allocation, so that one reduce moves both.  (The flag is the group's: a context's buffers are made once, by the
// first frame, and a context belongs to one group for its whole life.)
size_t frame_floats(const kdpt_ctx* c, bool moments) { return (moments ? 6 : 3) * (size_t)c->npix; }

int frame_buffers(kdpt_ctx* c, bool moments = false) {
  const size_t n3 = frame_floats(c, moments);
  if (!c->frames.reduce_stream) {
    int rc = create_stream(c, &c->frames.reduce_stream);
    if (rc) return rc;
  }
  for (int k = 0; k < 2; k++) {
    if (!c->frames.buf[k]) {
      HIP_TRY(c->frames.buf[k].alloc(n3));
      HIP_TRY(c->frames.ev[k].create_untimed());
      HIP_TRY(hipEventRecord(c->frames.ev[k], c->stream));
    }
  }
  if (!c->frames.sum && c->frames.rank == 0) HIP_TRY(c->frames.sum.alloc(n3));
  return KDPT_OK;
}

// A pageable host `out` is pinned in place for the frames' copies (hipHostRegister), so they run as queued
// instead of staging synchronously at every frame's enqueue (which would serialise frame f + 1's enqueue behind
// frame f's reduce); device memory, already pinned memory and failed registrations are left as they are.
void pin_host_out(kdpt_ctx* c, void* p, size_t bytes) {
  if (!p || !bytes) return;
  hipPointerAttribute_t a;
  if (hipPointerGetAttributes(&a, p) == hipSuccess && a.type != hipMemoryTypeUnregistered) return;
  (void)hipGetLastError();
  if (c->frames.host_reg.add(p, bytes) != hipSuccess) (void)hipGetLastError();
}

// Iterations of frame f for rank r of n: first, stride n, count.
void frame_share(int f, int spp, int n, int r, int* first, int* count) {
  *first = f * spp + 1 + r;
  *count = r < spp ? (spp - r + n - 1) / n : 0;
}

// Queue frame f's share of this rank into frame_buf[f & 1] (zeroed first, after its previous reduce), and make
// the reduce stream wait for it: the share's last add (c->pipe.acc_last), or, for a rank with no iterations in the
// frame, the zeroing itself, done on the reduce stream (which already follows the previous reduce).
int enqueue_frame(kdpt_ctx* c, int f, int spp, int pipeline, int batch, bool moments = false) {
  int rc = frame_buffers(c, moments);
  if (rc) return rc;
  float* fb = c->frames.buf[f & 1].get();
  int first, count;
  frame_share(f, spp, c->frames.nranks, c->frames.rank, &first, &count);
  const size_t nf = frame_floats(c, moments);
  if (count > 0) {
    IterationsCall call{first, count, c->frames.nranks, pipeline, batch, fb, c->frames.ev[f & 1]};
    // a frame that carries second moments: the share's squares go to the buffer's second half in the same adds
    if (moments) call.sumsq = fb + 3 * (size_t)c->npix;
    call.zero_floats = nf;
    if ((rc = enqueue_iterations(c, call))) return rc;
    HIP_TRY(hipStreamWaitEvent(c->frames.reduce_stream, c->pipe.acc_last, 0));
  } else {
    HIP_TRY(hipMemsetAsync(fb, 0, sizeof(float) * nf, c->frames.reduce_stream));
  }
  return KDPT_OK;
}

// Rank 0, after its frame image is in `sum`: add it into the context's image and copy it out.
int finish_frame(kdpt_ctx* c, const float* sum, float* out, int k, hipStream_t st) {
  const int n3 = 3 * c->npix;
  hipLaunchKernelGGL(k_accumulate_batch, dim3((n3 + 255) / 256), dim3(256), 0, st, c->image,
                     fill_parts<PartialImages>(&sum, 1), n3);
  HIP_TRY(hipGetLastError());
  c->accumulated = true;
  if (out) HIP_TRY(hipMemcpyAsync(out + (size_t)k * n3, sum, sizeof(float) * n3, hipMemcpyDefault, st));
  return KDPT_OK;
}

}  // namespace

// Everything the context owns goes with `delete c`, in reverse order of kdpt_ctx's members, once the streams are
// drained (a kdpt_render_frames that failed partway may have left a reduce queued) and the communicator released.
int kdpt_destroy(kdpt_ctx* c) {
  if (!c) return KDPT_OK;
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  c->pipe.drop_groups();  // (each group's stream drained first)
  if (c->frames.reduce_stream) (void)hipStreamSynchronize(c->frames.reduce_stream);
  release_comm(c);
  delete c;
  return KDPT_OK;
}

int kdpt_comm_library(char* path, int len) {
  if (!path || len < 1) return fail(KDPT_ERR_ARG, "bad arguments");
  const Rccl* R = rccl();
  if (!R) return fail(KDPT_ERR_UNSUPPORTED, "librccl.so.1 not found");
  // the file that actually provides ncclReduce (in a torch process: torch's own librccl, if loaded first)
  Dl_info info{};
  const char* f = dladdr(reinterpret_cast<void*>(R->reduce), &info) && info.dli_fname ? info.dli_fname : "?";
  snprintf(path, (size_t)len, "%s", f);
  return KDPT_OK;
}

int kdpt_comm_unique_id(unsigned char* id) {
  if (!id) return fail(KDPT_ERR_ARG, "null id");
  const Rccl* R = rccl();
  if (!R) return fail(KDPT_ERR_UNSUPPORTED, "librccl.so.1 not found");
  static_assert(sizeof(ncclUniqueId) == KDPT_COMM_ID_BYTES, "ncclUniqueId size");
  ncclUniqueId u;
  RCCL_TRY(R, R->getUniqueId(&u));
  memcpy(id, &u, sizeof u);
  return KDPT_OK;
}

int kdpt_comm_init(kdpt_ctx* c, int nranks, int rank, const unsigned char* id) {
  if (!c || nranks < 1 || rank < 0 || rank >= nranks) return fail(KDPT_ERR_ARG, "bad arguments");
  HIP_TRY(hipSetDevice(c->device));
  int rc = kdpt_synchronize(c);
  if (rc) return rc;
  release_comm(c);
  const Rccl* R = rccl();
  c->frames.nranks = nranks;
  c->frames.rank = rank;
  c->frames.external_reduce = nranks > 1 && !id;
  // (one rank with an id gets a communicator too: kdpt_render_frames then runs the same ncclReduce per frame
  // as on N GPUs, so one GPU exercises the multi-GPU path end to end)
  if (id) {
    if (!R) return fail(KDPT_ERR_UNSUPPORTED, "librccl.so.1 not found");
    ncclUniqueId u;
    memcpy(&u, id, sizeof u);
    ncclComm_t comm;
    RCCL_TRY(R, R->commInitRank(&comm, nranks, u, rank));
    c->frames.comm = comm;
    c->frames.owns_comm = true;
  }
  return KDPT_OK;
}

int kdpt_render_frames(kdpt_ctx* c, int first_frame, int frames, int spp, int pipeline, int batch, float* out) {
  if (!c || first_frame < 0 || frames < 0 || spp < 1) return fail(KDPT_ERR_ARG, "bad arguments");
  int rc;
  if (c->mom.on)
    return fail(KDPT_ERR_UNSUPPORTED,
                "kdpt_render_frames: the context keeps second moments (kdpt_set_moments), and frames reach the "
                "image through a cross-rank reduce that does not carry them; turn moments off first");
  HIP_TRY(hipSetDevice(c->device));
  const Rccl* R = c->frames.comm ? rccl() : nullptr;
  if (c->frames.nranks > 1 && !R && !c->frames.external_reduce) return fail(KDPT_ERR_ARG, "kdpt_comm_init first");
  const size_t n3 = 3 * (size_t)c->npix;
  if (c->frames.rank == 0 || c->frames.external_reduce) pin_host_out(c, out, sizeof(float) * n3 * (size_t)frames);
  for (int k = 0; k < frames; k++) {
    const int f = first_frame + k;
    if ((rc = enqueue_frame(c, f, spp, pipeline, batch))) return rc;
    float* fb = c->frames.buf[f & 1].get();
    // the frame's reduce and image add run on the reduce stream once its adds are done (enqueue_frame), while
    // the batch streams go on with the next frame's (other buffer)
    const hipStream_t rs = c->frames.reduce_stream;
    if ((rc = reduce_spin(c, rs))) return rc;
    const float* sum = fb;
    if (c->frames.external_reduce) {  // the caller reduces: every rank's share goes out as it is
      if (out) HIP_TRY(hipMemcpyAsync(out + (size_t)k * n3, fb, sizeof(float) * n3, hipMemcpyDefault, rs));
    } else {
      if (R) {
        RCCL_TRY(R, R->reduce(fb, c->frames.rank == 0 ? c->frames.sum.get() : nullptr, n3, ncclFloat32, ncclSum, 0,
                              (ncclComm_t)c->frames.comm, rs));
        sum = c->frames.sum.get();
      }
      if (c->frames.rank == 0 && (rc = finish_frame(c, sum, out, k, rs))) return rc;
    }
    HIP_TRY(hipEventRecord(c->frames.ev[f & 1], rs));
    // (entry points that read or write the image, and adds into it, follow the last reduce: join_accum)
    c->pipe.img_last = c->frames.ev[f & 1];
  }
  return KDPT_OK;
}
