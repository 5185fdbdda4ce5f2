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
% A bank (DESIGN.md section 9.8), for sources that move: rirs [nr x numChannels x numSources x numSets], and
%   x = f.push(src, setIndex)    setIndex ONE-based: [] (every source keeps its set; set 1 on a fresh object), a scalar (every
%                                source), [numSources] or [numSources x k], one index per source and block
% A change of set is cross-faded over the block that changes: its sample i goes to the new set with the gain i / blockSize
% (i = 1 .. blockSize) and to the old one with the rest; the first block after creation or reset does not fade.  The outputs equal
% sum_q sum_s fftfilt(rirs(:, c, q, s), g_sq .* s_q) with g_sq the gain of set s per sample of source q; a constant index gives
% the bits of the plain stream on that set.  numSets <= 65536; the response spectra of the whole bank <= 4 GiB.
    properties (SetAccess = private)
        handle = 0
        blockSize
        numSources
        numSets
    end
    methods
        function f = sourceFieldStream(rirs, blockSize)
            f.blockSize = blockSize;
            f.numSources = size(rirs, 3);
            f.numSets = size(rirs, 4);
            f.handle = emagls_mex('field_create', double(rirs), double(blockSize));
        end
        function out = push(f, src, setIndex)
            if nargin < 3, setIndex = []; end
            out = emagls_mex('field_push', f.handle, double(src), double(setIndex));
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
