// sift3d_device.hip -- the HIP runtime plumbing of the device C ABI (include/sift3d_amd.h): the error
// buffer every device unit reports through, and the device / memory / stream / event wrappers.
#include "sift3d_kernels_common.h"

thread_local char g_err[512] = "";

int fail(const char *what, hipError_t e, const char *file, int line)
{
    snprintf(g_err, sizeof(g_err), "%s: %s (%s:%d)", what, hipGetErrorString(e), file, line);
    fprintf(stderr, "sift3d_amd: %s\n", g_err);
    return SIFT3D_FAILURE;
}


extern "C" {

const char *sift3d_hip_last_error(void) { return g_err; }

int sift3d_hip_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess)
        return 0;
    return n;
}

int sift3d_amd_device_available(void) { return sift3d_hip_device_count() > 0; }

int sift3d_hip_current_device(void)
{
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess)
        return -1;
    return dev;
}

int sift3d_hip_set_device(int dev)
{
    HIPCHK(hipSetDevice(dev));
    return SIFT3D_SUCCESS;
}

void *sift3d_hip_malloc(size_t bytes)
{
    void *p = nullptr;
    hipError_t e = hipMalloc(&p, bytes ? bytes : 4);
    if (e != hipSuccess) {
        fail("hipMalloc", e, __FILE__, __LINE__);
        return nullptr;
    }
    return p;
}

void sift3d_hip_free(void *p)
{
    if (p)
        (void)hipFree(p);
}

void *sift3d_hip_host_alloc(size_t bytes)
{
    void *p = nullptr;
    hipError_t e = hipHostMalloc(&p, bytes ? bytes : 4, hipHostMallocDefault);
    if (e != hipSuccess) {
        fail("hipHostMalloc", e, __FILE__, __LINE__);
        return nullptr;
    }
    return p;
}

void *sift3d_hip_host_device_ptr(void *host)
{
    void *dev = nullptr;
    hipError_t e = hipHostGetDevicePointer(&dev, host, 0);
    if (e != hipSuccess) {
        fail("hipHostGetDevicePointer", e, __FILE__, __LINE__);
        return nullptr;
    }
    return dev;
}

void sift3d_hip_host_free(void *p)
{
    if (p)
        (void)hipHostFree(p);
}

int sift3d_hip_memcpy_h2d(void *d, const void *h, size_t bytes, void *stream)
{
    HIPCHK(hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, (hipStream_t)stream));
    return SIFT3D_SUCCESS;
}

int sift3d_hip_memcpy_d2h(void *h, const void *d, size_t bytes, void *stream)
{
    HIPCHK(hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, (hipStream_t)stream));
    return SIFT3D_SUCCESS;
}

int sift3d_hip_memcpy_d2d(void *d, const void *s, size_t bytes, void *stream)
{
    HIPCHK(hipMemcpyAsync(d, s, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return SIFT3D_SUCCESS;
}

int sift3d_hip_memcpy2d_d2h(void *h, size_t dpitch, const void *d, size_t spitch, size_t width,
                            size_t height, void *stream)
{
    HIPCHK(hipMemcpy2DAsync(h, dpitch, d, spitch, width, height, hipMemcpyDeviceToHost,
                            (hipStream_t)stream));
    return SIFT3D_SUCCESS;
}

int sift3d_hip_stream_wait_event(void *stream, void *ev)
{
    HIPCHK(hipStreamWaitEvent((hipStream_t)stream, (hipEvent_t)ev, 0));
    return SIFT3D_SUCCESS;
}

int sift3d_hip_memset(void *d, int byte, size_t bytes, void *stream)
{
    HIPCHK(hipMemsetAsync(d, byte, bytes, (hipStream_t)stream));
    return SIFT3D_SUCCESS;
}

void *sift3d_hip_stream_create(void)
{
    hipStream_t s = nullptr;
    hipError_t e = hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
    if (e != hipSuccess) {
        fail("hipStreamCreate", e, __FILE__, __LINE__);
        return nullptr;
    }
    return (void *)s;
}

// a stream whose kernels are dispatched ahead of those of ordinary streams (short, latency-bound
// work that runs beside device-filling kernels)
void *sift3d_hip_stream_create_high(void)
{
    hipStream_t s = nullptr;
    int lo = 0, hi = 0;
    (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
    hipError_t e = hipStreamCreateWithPriority(&s, hipStreamNonBlocking, hi);
    if (e != hipSuccess) {
        fail("hipStreamCreateWithPriority", e, __FILE__, __LINE__);
        return nullptr;
    }
    return (void *)s;
}

void sift3d_hip_stream_destroy(void *s)
{
    if (s)
        (void)hipStreamDestroy((hipStream_t)s);
}

int sift3d_hip_stream_sync(void *s)
{
    HIPCHK(hipStreamSynchronize((hipStream_t)s));
    return SIFT3D_SUCCESS;
}

void *sift3d_hip_event_create(void)
{
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) != hipSuccess)
        return nullptr;
    return (void *)e;
}

void sift3d_hip_event_destroy(void *e)
{
    if (e)
        (void)hipEventDestroy((hipEvent_t)e);
}

int sift3d_hip_event_record(void *e, void *s)
{
    HIPCHK(hipEventRecord((hipEvent_t)e, (hipStream_t)s));
    return SIFT3D_SUCCESS;
}

double sift3d_hip_event_elapsed_ms(void *a, void *b)
{
    float ms = 0.f;
    if (hipEventSynchronize((hipEvent_t)b) != hipSuccess)
        return -1.0;
    if (hipEventElapsedTime(&ms, (hipEvent_t)a, (hipEvent_t)b) != hipSuccess)
        return -1.0;
    return (double)ms;
}

} // extern "C"
