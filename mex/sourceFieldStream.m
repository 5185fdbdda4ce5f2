classdef sourceFieldStream < handle
% Dry source signals through array room responses, a block at a time on the GPU (DESIGN.md section 9.7): what
% fftfilt(srir.rir, sig) does offline (testEMagLs.m:66-70), for a head that moves while the sound plays.
%   f = sourceFieldStream(rirs, blockSize)    rirs [nr x numChannels], or [nr x numChannels x numSources]; real or complex
%   x = f.push(src)      src [k*blockSize x numSources] real -> x [k*blockSize x numChannels], complex for a complex response
%   f.reset()    zero history        delete(f)    releases the device memory
% Concatenating everything pushed for source q into s_q, the concatenated outputs equal sum_q fftfilt(rirs(:, c, q), s_q) to
% rounding; nothing is held back.  Push x into a binauralDecodeStream or a binauralDecodeGroup (created with complexInput for a
% complex response; responses in the microphone domain go into one with an encoder) together with the head orientation of the
% block: the chain is source -> room -> rotation -> filters.  blockSize: a power of two from 64 to 2048; numSources <= 16,
% numChannels <= 256, nr <= 1048576.
    properties (SetAccess = private)
        handle = 0
        blockSize
        numSources
    end
    methods
        function f = sourceFieldStream(rirs, blockSize)
            f.blockSize = blockSize;
            f.numSources = size(rirs, 3);
            f.handle = emagls_mex('field_create', double(rirs), double(blockSize));
        end
        function out = push(f, src)
            out = emagls_mex('field_push', f.handle, double(src));
        end
        function reset(f)
            emagls_mex('field_reset', f.handle);
        end
        function delete(f)
            if f.handle > 0
                emagls_mex('field_destroy', f.handle);
                f.handle = 0;
            end
        end
    end
end
